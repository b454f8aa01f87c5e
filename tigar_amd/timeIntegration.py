"""
The ``timeIntegration`` module
------------------------------
Time integrators of tIGAr/timeIntegration.py on device vectors: ``BackwardEulerIntegrator``,
``GeneralizedAlphaIntegrator``, ``LoadStepper`` and ``x_alpha`` with the reference's constructor signatures and
attributes, and ``LinearTransientProblem``, a driver for linear first- and second-order problems that keeps the
whole state on the device between steps.

The reference states its formulas as UFL expressions in the unknown ``Function`` and the functions of the previous
step.  There is no UFL here: ``xdot()``, ``xddot()``, ``x_alpha()`` ... return a ``LinearCombination``, a list of
``(coefficient, vector)`` terms that can be added, scaled, split into "coefficient of the unknown" and "the rest" (what
a linear problem needs to form its matrix and right-hand side) and evaluated on the device in one pass
(csrc/tg_timeint.hip: ``tg_vec_lincomb``).  ``advance()`` is one fused in-place kernel (``tg_state_advance``).

``NonlinearTransientProblem`` drives nonlinear structural dynamics -- a shell or solid residual with inertia, mass damping
and a rigid plane (``forms.DynamicResidual``, csrc/tg_dynamics.hip) -- with one Newton solve per step.
``FlowTransientProblem`` does the same for the first-order system of the stabilised incompressible flow
(``forms.FlowResidual``, csrc/tg_flow.hip), read at the alpha level.

``LinearDGSpaceTimeIntegrator`` is not provided: it is a helper that arranges UFL forms over a time slab and has no
numerics of its own.
"""
import time as _time

from . import device as _dev
from .device import DeviceVector


def _vec_of(f):
    """the vector behind a ``Function`` (or the object itself: a ``DeviceVector``, or any stand-in on the host)"""
    vector = getattr(f, "vector", None)
    return vector() if callable(vector) else f


class LinearCombination(object):
    """``sum_i c_i v_i`` of vectors (``Function`` / ``DeviceVector``).  Terms on the same vector are merged; the order of
    first appearance is kept, so an expression evaluates in a fixed order."""

    def __init__(self, terms=()):
        self.terms = []
        for c, v in terms:
            self._add(float(c), v)

    def _add(self, c, v):
        key = _vec_of(v)
        for i, (ci, vi) in enumerate(self.terms):
            if _vec_of(vi) is key:
                self.terms[i] = (ci + c, vi)
                return
        self.terms.append((c, v))

    @staticmethod
    def of(v):
        return v if isinstance(v, LinearCombination) else LinearCombination([(1.0, v)])

    def __add__(self, other):
        return LinearCombination(self.terms + LinearCombination.of(other).terms)

    __radd__ = __add__

    def __neg__(self):
        return self * -1.0

    def __sub__(self, other):
        return self + (-LinearCombination.of(other))

    def __rsub__(self, other):
        return LinearCombination.of(other) + (-self)

    def __mul__(self, a):
        if isinstance(a, (LinearCombination, DeviceVector)) or hasattr(a, "vector"):
            return NotImplemented
        a = float(a)
        return LinearCombination([(a * c, v) for c, v in self.terms])

    __rmul__ = __mul__

    def __truediv__(self, a):
        return self * (1.0 / float(a))

    def coefficient(self, v):
        key = _vec_of(v)
        return sum(c for c, w in self.terms if _vec_of(w) is key)

    def split(self, v):
        """``(coefficient of v, the rest)``"""
        key = _vec_of(v)
        return self.coefficient(v), LinearCombination([(c, w) for c, w in self.terms if _vec_of(w) is not key])

    def evaluate(self, out=None):
        """The value as a ``DeviceVector``: one ``tg_vec_lincomb`` call for up to 8 terms, chunks of 7 more after that.
        ``out`` may be one of the vectors of the expression."""
        terms = [(c, _vec_of(v)) for c, v in self.terms]
        if not terms:
            if out is None:
                raise ValueError("LinearCombination.evaluate: an empty expression has no size; pass out=")
            out = _vec_of(out)
            out.zero()
            return out
        dst = _vec_of(out) if out is not None else DeviceVector(terms[0][1].size(), zero=False)
        acc = dst
        if len(terms) > 8 and any(v is dst for _, v in terms):
            acc = DeviceVector(dst.size(), zero=False)       # (later chunks would read a dst that is already overwritten)
        _dev.vec_lincomb(acc, [c for c, _ in terms[:8]], [v for _, v in terms[:8]])
        for i in range(8, len(terms), 7):
            chunk = terms[i:i + 7]
            _dev.vec_lincomb(acc, [1.0] + [c for c, _ in chunk], [acc] + [v for _, v in chunk])
        if acc is not dst:
            dst[:] = acc
        return dst


def x_alpha(alpha, x, x_old):
    """The ``alpha``-level quantity ``alpha*x + (1 - alpha)*x_old``."""
    return alpha * LinearCombination.of(x) + (1.0 - alpha) * LinearCombination.of(x_old)


class BackwardEulerIntegrator(object):
    """Backward Euler formulas for first- and second-order ODE systems.  ``oldFunctions``: ``[x_old]`` (first order) or
    ``[x_old, xdot_old]`` (second order); ``t`` is the initial time, ``self.t`` the time of the step being computed."""

    def __init__(self, DELTA_T, x, oldFunctions, t=0.0):
        self.systemOrder = len(oldFunctions)
        if self.systemOrder not in (1, 2):
            raise ValueError("BackwardEulerIntegrator: one or two old functions are expected, not %d" % self.systemOrder)
        self.DELTA_T = DELTA_T
        self.x = x
        self.x_old = oldFunctions[0]
        if self.systemOrder == 2:
            self.xdot_old = oldFunctions[1]
        self.t = t + float(DELTA_T)

    def xdot(self):
        """velocity of the current step"""
        return (LinearCombination.of(self.x) - self.x_old) / float(self.DELTA_T)

    def xddot(self):
        """acceleration of the current step"""
        return (self.xdot() - self.xdot_old) / float(self.DELTA_T)

    def advance(self):
        """The data of the current step become those of the previous one (on the device, in place)."""
        if self.systemOrder == 2:
            h = 1.0 / float(self.DELTA_T)
            _dev.state_advance([h, -h, 0.0, 0.0, 0.0, 0.0, 0.0], _vec_of(self.x), _vec_of(self.x_old), _vec_of(self.xdot_old))
        else:
            _vec_of(self.x_old)[:] = _vec_of(self.x)
        self.t += float(self.DELTA_T)


class LoadStepper(object):
    """Time "integrator" of a problem without time derivatives: keeps the (pseudo)time that parameterises a load.
    ``t`` is the plain float ``tval`` (the reference wraps it in a dolfin ``Expression``)."""

    def __init__(self, DELTA_T, t=0.0):
        self.DELTA_T = DELTA_T
        self.tval = t
        self.t = t
        self.advance()

    def advance(self):
        self.tval += float(self.DELTA_T)
        self.t = self.tval


class GeneralizedAlphaIntegrator(object):
    """Generalized-alpha formulas (Chung & Hulbert 1993; Jansen, Whiting & Hulbert 2000 for first-order systems) with
    spectral radius ``RHO_INF`` in the limit of large time steps.  ``oldFunctions``: ``[x_old, xdot_old]`` (first-order
    system) or ``[x_old, xdot_old, xddot_old]`` (second order).  ``useFirstOrderAlphaM``: the first-order alpha_m for a
    second-order system.  ``RHO_INF = 1`` is the implicit midpoint rule.  The initial acceleration (first order: velocity)
    over-determines the problem and should be compatible with the other data and the governing equation."""

    def __init__(self, RHO_INF, DELTA_T, x, oldFunctions, t=0.0, useFirstOrderAlphaM=False):
        self.RHO_INF = RHO_INF
        self.DELTA_T = DELTA_T
        self.systemOrder = len(oldFunctions) - 1
        if self.systemOrder not in (1, 2):
            raise ValueError("GeneralizedAlphaIntegrator: two or three old functions are expected, not %d" % len(oldFunctions))
        # Both alphas are multiples of 1 / (1 + rho): alpha_f = 1, alpha_m = 2 - rho (Chung & Hulbert) or (3 - rho) / 2
        # (Jansen et al.) of it.  Second-order accuracy fixes gamma = 1/2 + alpha_m - alpha_f, unconditional stability
        # with the most high-frequency damping beta = ((1/2 + gamma) / 2)^2.
        rho = float(RHO_INF)
        self.ALPHA_F = 1.0 / (1.0 + rho)
        first_order = useFirstOrderAlphaM or self.systemOrder == 1
        self.ALPHA_M = self.ALPHA_F * (1.5 - 0.5 * rho if first_order else 2.0 - rho)
        self.GAMMA = 0.5 + self.ALPHA_M - self.ALPHA_F
        self.BETA = (0.5 * (0.5 + self.GAMMA)) ** 2
        self.x = x
        self.x_old = oldFunctions[0]
        self.xdot_old = oldFunctions[1]
        if self.systemOrder == 2:
            self.xddot_old = oldFunctions[2]
        self.t = t + float(DELTA_T)

    # The Newmark relations between the levels n and n+1 (h = DELTA_T):
    #     (N1)  y     = y_old + h ((1 - gamma) ydot_old + gamma ydot)              y = x (first order), y = xdot (second)
    #     (N2)  x     = x_old + h xdot_old + h^2 ((1/2 - beta) xddot_old + beta xddot)
    # The methods below are (N1) and (N2) solved for the rates of level n+1.
    def _rate_coefficients(self):
        """(r, -r, s): (N1) solved for the new rate, ydot = r y - r y_old + s ydot_old with r = 1 / (gamma h) and
        s = 1 - 1 / gamma"""
        r = 1.0 / (self.GAMMA * float(self.DELTA_T))
        return r, -r, 1.0 - 1.0 / self.GAMMA

    def _xdot_coefficients(self):
        """(c0, c1, c2, c3): xdot = c0 x + c1 x_old + c2 xdot_old + c3 xddot_old.  Second order: (N2) gives
        xddot = (x - x_old - h xdot_old) / (beta h^2) - (1 / (2 beta) - 1) xddot_old; put into (N1) with q = gamma / beta,
        the xddot_old terms (1 - gamma) - gamma (1 / (2 beta) - 1) collapse to 1 - q / 2."""
        if self.systemOrder == 1:
            return self._rate_coefficients() + (0.0,)
        h, q = float(self.DELTA_T), self.GAMMA / self.BETA
        return q / h, -q / h, 1.0 - q, h * (1.0 - 0.5 * q)

    def _xddot_coefficients(self):
        """(c4, c5, c6): xddot = c4 xdot + c5 xdot_old + c6 xddot_old, (N1) on the velocity"""
        return self._rate_coefficients()

    def xdot(self):
        """velocity at level n+1 in terms of the unknown and the data of the previous step"""
        c = self._xdot_coefficients()
        e = c[0] * LinearCombination.of(self.x) + c[1] * LinearCombination.of(self.x_old) + c[2] * LinearCombination.of(self.xdot_old)
        if self.systemOrder == 2:
            e = e + c[3] * LinearCombination.of(self.xddot_old)
        return e

    def xddot(self):
        """acceleration at level n+1 (second-order systems only)"""
        c = self._xddot_coefficients()
        return c[0] * self.xdot() + c[1] * LinearCombination.of(self.xdot_old) + c[2] * LinearCombination.of(self.xddot_old)

    def x_alpha(self):
        return x_alpha(self.ALPHA_F, self.x, self.x_old)

    def xdot_alpha(self):
        alpha = self.ALPHA_M if self.systemOrder == 1 else self.ALPHA_F
        return x_alpha(alpha, self.xdot(), self.xdot_old)

    def xddot_alpha(self):
        """alpha-level acceleration (second-order systems only)"""
        return x_alpha(self.ALPHA_M, self.xddot(), self.xddot_old)

    def sameVelocityPredictor(self):
        """Predictor of the unknown that keeps the velocity (``xdot`` of a second-order system, ``x`` of a first-order
        one, for which it is ``x_old`` itself)."""
        if self.systemOrder == 1:
            return LinearCombination.of(self.x_old)
        # xdot = xdot_old in (N1) asks for xddot = (1 - 1 / gamma) xddot_old; (N2) with that acceleration leaves
        # h^2 (1/2 - beta / gamma) on xddot_old
        h = float(self.DELTA_T)
        return LinearCombination([(1.0, self.x_old), (h, self.xdot_old),
                                  (h * h * (0.5 - self.BETA / self.GAMMA), self.xddot_old)])

    def advance(self):
        """The data of the current step become those of the previous one: one fused kernel, in place (an entry's values
        are in registers before any is overwritten, so no copies are made)."""
        c = list(self._xdot_coefficients())
        if self.systemOrder == 2:
            _dev.state_advance(c + list(self._xddot_coefficients()), _vec_of(self.x), _vec_of(self.x_old),
                               _vec_of(self.xdot_old), _vec_of(self.xddot_old))
        else:
            _dev.state_advance(c + [0.0, 0.0, 0.0], _vec_of(self.x), _vec_of(self.x_old), _vec_of(self.xdot_old))
        self.t += float(self.DELTA_T)


class LinearTransientProblem(object):
    """Transient response of a linear problem on an ``ExtractedSpline``,

        order 2:  M xddot + C xdot + K x = f(t),   C = a_M M + a_K K (Rayleigh, ``damping=(a_M, a_K)``)
        order 1:  M xdot + K x = f(t),

    by the generalized-alpha method (``scheme="generalized_alpha"``, ``RHO_INF``) or backward Euler
    (``scheme="backward_euler"``).  K and M are assembled once; the time step is constant, so the effective matrix
    ``K_eff = c_K K + c_M M`` is built once as well (it keeps the tensor structure and the symmetry certificate of K and
    M: ``PETScKrylovSolver("cg", "fast_diagonalization")`` serves it).  Per step: two ``tg_vec_lincomb`` form what
    multiplies M and K on the right-hand side, ``rhs = f(t_alpha) - M w_M - K w_K`` is formed by two products and two axpy
    (or by one ``tg_spmv_pair``: ``FUSED_RHS``), the solve
    goes through ``spline.linearSolver`` (default solver when None; a Krylov solver is started from the same-velocity
    predictor) and ``advance()`` is one kernel.  Nothing leaves the device between steps.

    ``load``: None or a callable ``t -> form`` (anything ``spline.assembleVector`` takes) or ``t -> DeviceVector`` of IGA
    dofs.  ``x0`` / ``xdot0``: IGA-dof ``DeviceVector`` s, FE ``Function`` s (brought over by ``spline.FEtoIGA``) or callables
    on the physical points ``[npts, nsd] -> [npts]`` (L2-projected by ``spline.projectDofs(.., applyBCs=True,
    rational=rational)``: ``rational=True`` with stiffness and mass forms of the rational space); None = 0,
    except ``xdot0=None`` of a first-order generalized-alpha problem: solved from ``M xdot0 = f(t0) - K x0``.  For order 2
    the initial acceleration is solved from ``M a0 = f(t0) - C xdot0 - K x0``.

    ``x``, ``xdot``, ``xddot``: the state at time ``t`` (IGA dofs); ``u``: FE ``Function`` u = M x, refreshed by
    ``prolong()``; ``energy()``; ``integrator``; ``last``: iterations and seconds per phase of the last step.  The seconds
    cost four device synchronisations per step; ``prob.timing = False`` drops them (the seconds are then None) and a
    run of steps is enqueued without the host waiting, as far as the solver allows.

    With ``spline.linearSolver = None`` and a system small enough for the default banded direct solver, every step
    factorises ``K_eff`` again: the direct solvers keep no factors between calls.  For many steps set a Krylov solver
    (``PETScKrylovSolver("cg", "fast_diagonalization")`` on an unmapped patch), whose setup is kept on ``K_eff``."""

    # rhs = f - M w_M - K w_K through the fused pair product (True) or two products and two axpy (False).  The pair product
    # moves fewer bytes (20 B per stored entry against 2 x 12 B) but is the slower of the two on the MI355X from 48^3 p = 3
    # elements on: 0.474 ms against 0.427 ms at 64^3 (profiles/timeint_bench.jsonl, tools/timeint_bench.py); it wins only
    # where launches dominate (32^3: 0.049 against 0.070 ms).  Hence two products.
    FUSED_RHS = False
    # fill the seconds of ``last`` (four device synchronisations per step)
    timing = True

    def __init__(self, spline, stiffness, mass, order=2, scheme="generalized_alpha", RHO_INF=0.5, DELTA_T=None, damping=None,
                 load=None, x0=None, xdot0=None, t=0.0, rational=False):
        if order not in (1, 2):
            raise ValueError("LinearTransientProblem: order must be 1 or 2, not %r" % (order,))
        if scheme not in ("generalized_alpha", "backward_euler"):
            raise ValueError("LinearTransientProblem: scheme must be 'generalized_alpha' or 'backward_euler', not %r" % (scheme,))
        if DELTA_T is None or not float(DELTA_T) > 0.0:
            raise ValueError("LinearTransientProblem: DELTA_T must be positive, not %r" % (DELTA_T,))
        if scheme == "generalized_alpha" and not 0.0 <= float(RHO_INF) <= 1.0:
            raise ValueError("LinearTransientProblem: RHO_INF must lie in [0, 1], not %r" % (RHO_INF,))
        if damping is not None and (order != 2 or len(damping) != 2):
            raise ValueError("LinearTransientProblem: damping=(a_M, a_K) belongs to a second-order problem")
        if spline._distributed():
            raise NotImplementedError("LinearTransientProblem: several ranks are not supported")
        if spline._caller_ordered():
            raise NotImplementedError("LinearTransientProblem: a spline with the caller's FE dof order (feOrder) is not supported")
        self.spline, self.order, self.scheme, self.load = spline, int(order), scheme, load
        self.rational = bool(rational)        # the space callable initial data are projected in (that of the forms handed in)
        self.DELTA_T = dt = float(DELTA_T)
        self.damping = (0.0, 0.0) if damping is None else (float(damping[0]), float(damping[1]))
        self.K = spline.assembleMatrix(stiffness)
        self.Mm = spline.assembleMatrix(mass)
        if not isinstance(self.K, _dev.DeviceCSR) or not isinstance(self.Mm, _dev.DeviceCSR):
            raise NotImplementedError("LinearTransientProblem: stiffness and mass must be resident CSR matrices (row-block "
                                      "matrices of the streamed engines are not supported)")
        if self.K.shape != self.Mm.shape or self.K.shape[0] != self.K.shape[1]:
            raise ValueError("LinearTransientProblem: stiffness %s and mass %s differ in shape" % (self.K.shape, self.Mm.shape))
        # built whatever FUSED_RHS says: creating the pair is also the pattern check of mass against stiffness (one
        # comparison on the device; ValueError when they differ), which K.combine and the shared w_M / w_K rely on
        self._pair = _dev.CSRPair(self.Mm, self.K)
        n = self.n = self.K.shape[0]
        self._zero = spline.zeroDofs
        self._x = DeviceVector(n)
        self._x_old = self._initial(x0)
        old = [self._x_old]
        gen_alpha = scheme == "generalized_alpha"
        if gen_alpha or order == 2:
            self._xdot_old = self._initial(xdot0)
            old.append(self._xdot_old)
        if gen_alpha and order == 2:
            self._xddot_old = DeviceVector(n)
            old.append(self._xddot_old)
        if gen_alpha:
            self.integrator = it = GeneralizedAlphaIntegrator(float(RHO_INF), dt, self._x, old, t=float(t))
        else:
            self.integrator = it = BackwardEulerIntegrator(dt, self._x, old, t=float(t))
        self._x[:] = self._x_old
        # what multiplies M and what multiplies K in the equation of a step, as expressions in the unknown and the old state
        a_M, a_K = self.damping
        X = LinearCombination.of(self._x)
        if gen_alpha:
            e_K = it.x_alpha() + a_K * it.xdot_alpha() if order == 2 else it.x_alpha()
            e_M = it.xddot_alpha() + a_M * it.xdot_alpha() if order == 2 else it.xdot_alpha()
        else:
            e_K = X + a_K * it.xdot() if order == 2 else X
            e_M = it.xddot() + a_M * it.xdot() if order == 2 else it.xdot()
        self.c_M, self._w_M = e_M.split(self._x)
        self.c_K, self._w_K = e_K.split(self._x)
        self.K_eff = self.K.combine(self.c_K, self.Mm, self.c_M)
        self._wM, self._wK, self._rhs = DeviceVector(n), DeviceVector(n), DeviceVector(n)
        self.u = None
        self.last = None
        self.steps_done = 0
        # compatible initial rate: the acceleration of a second-order problem, the velocity of a first-order one
        if gen_alpha and order == 2 and not (x0 is None and xdot0 is None and load is None):
            self._wM.zero()
            _dev.vec_lincomb(self._wM, [a_M], [self._xdot_old])
            _dev.vec_lincomb(self._wK, [1.0, a_K], [self._x_old, self._xdot_old])
            self._solve_mass(self._xddot_old, float(t))
        elif gen_alpha and order == 1 and xdot0 is None and not (x0 is None and load is None):
            self._wM.zero()
            self._wK[:] = self._x_old
            self._solve_mass(self._xdot_old, float(t))

    # -- state
    @property
    def t(self):
        """time of the state ``x``, ``xdot``, ``xddot``"""
        return self.integrator.t - self.DELTA_T

    @property
    def x(self):
        return self._x_old

    @property
    def xdot(self):
        return getattr(self, "_xdot_old", None)

    @property
    def xddot(self):
        return getattr(self, "_xddot_old", None)

    def _initial(self, v):
        out = DeviceVector(self.n)
        if v is None:
            return out
        if hasattr(v, "vector"):
            v = self.spline.FEtoIGA(v)
        elif callable(v):
            v = self.spline.projectDofs(v, applyBCs=True, rational=self.rational)     # a function of x: its L2 projection
        if not isinstance(v, DeviceVector) or v.size() != self.n:
            raise ValueError("LinearTransientProblem: initial data must be a DeviceVector of %d IGA dofs, an FE Function or a "
                             "callable" % self.n)
        out[:] = v
        out.zero_entries(self._zero)
        return out

    def _load_vector(self, t):
        if self.load is None:
            return None
        f = self.load(t)
        if isinstance(f, DeviceVector):
            if f.size() != self.n:
                raise ValueError("LinearTransientProblem: the load has %d entries, the problem %d dofs" % (f.size(), self.n))
            return f
        return self.spline.assembleVector(f)

    def _residual(self, f):
        """self._rhs = f - Mm self._wM - K self._wK, zero on the zero dofs"""
        if self.FUSED_RHS:
            self._pair.mult(self._wM, self._wK, y0=f, y=self._rhs)
        else:
            if f is None:
                self._rhs.zero()
            else:
                self._rhs[:] = f
            tmp = self.__dict__.setdefault("_tmp", DeviceVector(self.n))
            self._rhs.axpy(-1.0, self.Mm.mult(self._wM, tmp))
            self._rhs.axpy(-1.0, self.K.mult(self._wK, tmp))
        self._rhs.zero_entries(self._zero)

    def _solver(self):
        from .common import _default_linear_solver
        s = self.spline.linearSolver
        return s if s is not None else _default_linear_solver()

    def _solve_mass(self, out, t):
        self._residual(self._load_vector(t))
        self._solver().solve(self.Mm, out, self._rhs)
        out.zero_entries(self._zero)

    # -- stepping
    def _clock(self):
        """host time after the device has caught up; nothing (no synchronisation) when ``timing`` is off"""
        if not self.timing:
            return None
        _dev.sync()
        return _time.perf_counter()

    def step(self, n=1):
        """advances the state by ``n`` steps of ``DELTA_T``"""
        it = self.integrator
        for _ in range(int(n)):
            t0 = self._clock()
            self._w_M.evaluate(out=self._wM)
            self._w_K.evaluate(out=self._wK)
            t_eval = it.t - (1.0 - it.ALPHA_F) * self.DELTA_T if self.scheme == "generalized_alpha" else it.t
            self._residual(self._load_vector(t_eval))
            t1 = self._clock()
            solver = self._solver()
            params = getattr(solver, "parameters", None)
            krylov = isinstance(params, dict) and "nonzero_initial_guess" in params
            if krylov:
                saved = params["nonzero_initial_guess"]
                params["nonzero_initial_guess"] = True
                if self.scheme == "generalized_alpha":
                    it.sameVelocityPredictor().evaluate(out=self._x)
                else:
                    self._x[:] = self._x_old
            try:
                its = solver.solve(self.K_eff, self._x, self._rhs)
            finally:
                if krylov:
                    params["nonzero_initial_guess"] = saved
            self._x.zero_entries(self._zero)
            t2 = self._clock()
            it.advance()
            t3 = self._clock()
            last = getattr(solver, "last", None)
            self.last = {"iterations": last.get("iterations", its) if isinstance(last, dict) else its,
                         "rhs_seconds": t1 - t0 if self.timing else None, "solve_seconds": t2 - t1 if self.timing else None,
                         "advance_seconds": t3 - t2 if self.timing else None}
            self.steps_done += 1
        return self

    def prolong(self):
        """``u = M x`` as an FE ``Function`` (kept in ``self.u``)"""
        from .common import Function
        if self.u is None:
            self.u = Function(self.spline.V)
        self.spline.M.mult(self._x_old, self.u.vector())
        self.u.invalidate_ghosts()
        return self.u

    def energy(self):
        """order 2: ``xdot^T M xdot / 2 + x^T K x / 2``; order 1: ``x^T M x / 2``"""
        tmp = self.__dict__.setdefault("_tmp", DeviceVector(self.n))
        if self.order == 1:
            return 0.5 * self._x_old.inner(self.Mm.mult(self._x_old, tmp))
        e = 0.5 * self._xdot_old.inner(self.Mm.mult(self._xdot_old, tmp))
        return e + 0.5 * self._x_old.inner(self.K.mult(self._x_old, tmp))


def _set_initial_state(who, spline, f, v, constants_rational=None):
    """Initial data ``v`` into the FE Function ``f``: an FE Function (copied), a DeviceVector of IGA dofs (prolonged by M) or None
    (``f`` stays as it is).  ``constants_rational`` not None: nF numbers are taken as well, a constant vector -- with True the
    nodal values are w_i c, the homogeneous representation of the constant in the rational space.  Anything else: ValueError."""
    import numpy
    fv = _vec_of(f)
    ndofs = spline.M.shape[1]
    if v is None:
        return
    if hasattr(v, "vector"):
        if _vec_of(v).size() != fv.size():
            raise ValueError("%s: an initial Function of %d nodal values, the space has %d" % (who, _vec_of(v).size(), fv.size()))
        fv[:] = _vec_of(v)
    elif isinstance(v, DeviceVector):
        if v.size() != ndofs:
            raise ValueError("%s: initial data of %d values, the spline has %d IGA dofs" % (who, v.size(), ndofs))
        spline.M.mult(v, fv)
    else:
        nF = len(spline.V.grids)
        c = numpy.asarray(v, dtype=numpy.float64).ravel() if constants_rational is not None else None
        if c is None or c.size != nF:
            raise ValueError("%s: initial data must be an FE Function%s a DeviceVector of %d IGA dofs%s"
                             % (who, "," if c is not None else " or", ndofs, " or %d numbers" % nF if c is not None else ""))
        n = fv.size() // nF
        w = _vec_of(spline.cpFuncs[-1]).get_local() if constants_rational else numpy.ones(n)
        fv.set_local(numpy.concatenate([ci * w for ci in c]))
    if hasattr(f, "invalidate_ghosts"):
        f.invalidate_ghosts()


class NonlinearTransientProblem(object):
    """Nonlinear structural dynamics on an ``ExtractedSpline``, the flow of demos/kl-shell-svk/dynamic-tspline.py:100-293:

        rho (yddot + a_M ydot) + D psi(y) = loads + contact        (``forms.DynamicResidual``)

    by the generalized-alpha method (``scheme="generalized_alpha"``, ``RHO_INF``) or backward Euler
    (``scheme="backward_euler"``), one ``spline.solveNonlinearVariationalProblem`` per step.  ``static``: a
    ``forms.ShellResidual`` or ``forms.HyperelasticResidual``; its ``u`` is the unknown y of the step being computed.
    ``density``: mass per unit reference measure; ``mass_damping`` = a_M; ``contact``: a ``forms.PlanePenalty`` or None.
    The problem owns ``y_old``, ``ydot_old``, ``yddot_old`` (FE Functions), ``integrator`` and ``dyn`` (the
    ``DynamicResidual``, which returns R / alpha_f and (dR/dy) / alpha_f: ``dyn.scale``).

    ``step(n)``, per step: the same-velocity predictor into y (one ``tg_vec_lincomb``), the Newton solve, ``advance()`` (one
    ``tg_state_advance``).  The Newton test is relative to the first norm, which fails when the predictor is already
    converged (a body at rest): with ``absoluteTolerance`` > 0 the step also ends, without a Newton step, when the first
    ||M^T R / alpha_f|| <= absoluteTolerance; 0.0 is the reference's behaviour.

    ``y0`` / ``ydot0``: FE Functions, IGA-dof ``DeviceVector`` s (prolonged by M), nF numbers (a constant vector; with
    ``rational=True`` of ``static`` the nodal values are w_i c, the homogeneous representation of the constant) or None = 0.
    ``initial_acceleration=True`` solves rho M a0 = -R_static(y0) - rho a_M M ydot0 once (the value-value form as the mass
    matrix; the penalty is not in it); False leaves a0 = 0, as the demo does.

    ``y``, ``ydot``, ``yddot``: the state at time ``t`` (FE Functions; ``yddot`` None for backward Euler); ``t_alpha``: the
    time the loads of the step being computed are read at; ``energy()``; ``last``: {"newton": relative norms, "iterations",
    "active_points", "assembly_seconds", "solve_seconds"} of the last step, the seconds None when ``timing`` is off (they
    cost three device synchronisations per Newton iteration)."""

    timing = True

    def __init__(self, spline, static, density, DELTA_T, RHO_INF=0.5, scheme="generalized_alpha", mass_damping=0.0, contact=None,
                 y0=None, ydot0=None, t=0.0, initial_acceleration=True, absoluteTolerance=0.0):
        from . import forms as _forms
        from .common import Function
        who = "NonlinearTransientProblem"
        if scheme not in ("generalized_alpha", "backward_euler"):
            raise ValueError("%s: scheme must be 'generalized_alpha' or 'backward_euler', not %r" % (who, scheme))
        if DELTA_T is None or not float(DELTA_T) > 0.0:
            raise ValueError("%s: DELTA_T must be positive, not %r" % (who, DELTA_T))
        if scheme == "generalized_alpha" and not 0.0 <= float(RHO_INF) <= 1.0:
            raise ValueError("%s: RHO_INF must lie in [0, 1], not %r" % (who, RHO_INF))
        if not float(absoluteTolerance) >= 0.0:
            raise ValueError("%s: absoluteTolerance = %r must not be negative" % (who, absoluteTolerance))
        if spline._distributed():
            raise NotImplementedError("%s: several ranks are not supported" % who)
        if spline._caller_ordered():
            raise NotImplementedError("%s: a spline with the caller's FE dof order (feOrder) is not supported" % who)
        if not isinstance(static, (_forms.ShellResidual, _forms.HyperelasticResidual)):
            raise NotImplementedError("%s: static = %r; a ShellResidual or a HyperelasticResidual carries the law" % (who, static))
        self.spline, self.static, self.scheme = spline, static, scheme
        self.DELTA_T, self.absoluteTolerance = float(DELTA_T), float(absoluteTolerance)
        self._y = static.u
        V = spline.V
        self.y_old, self.ydot_old = Function(V), Function(V)
        self._set_initial(self.y_old, y0)
        self._set_initial(self.ydot_old, ydot0)
        if scheme == "generalized_alpha":
            self.yddot_old = Function(V)
            self.integrator = GeneralizedAlphaIntegrator(float(RHO_INF), self.DELTA_T, self._y, [self.y_old, self.ydot_old, self.yddot_old],
                                                         t=float(t))
        else:
            self.yddot_old = None
            self.integrator = BackwardEulerIntegrator(self.DELTA_T, self._y, [self.y_old, self.ydot_old], t=float(t))
        _vec_of(self._y)[:] = _vec_of(self.y_old)
        self.dyn = _forms.DynamicResidual(static, self.integrator, density, mass_damping=mass_damping, contact=contact)
        self._tangent = self.dyn.tangent()
        self.last = None
        self.steps_done = 0
        if initial_acceleration and self.yddot_old is not None:
            self._initial_acceleration()

    def _set_initial(self, f, v):
        """``v`` (an FE Function, IGA dofs, nF numbers or None) into the FE Function ``f``"""
        _set_initial_state("NonlinearTransientProblem", self.spline, f, v, constants_rational=bool(self.static.rational))

    def _initial_acceleration(self):
        """rho M a0 = -R_static(y0) - rho a_M M ydot0 in the IGA dofs; a0 = M (the solution) into ``yddot_old``"""
        spline, dyn = self.spline, self.dyn
        mass = dyn.mass_form().assemble_matrix(spline.V)
        b = self.static.assemble_vector(spline.V)                   # (static.u = y = y0)
        if dyn.mass_damping != 0.0:
            b.axpy(dyn.mass_damping, mass.mult(_vec_of(self.ydot_old)))
        _dev.vec_lincomb(b, [-1.0], [b])
        spline.solveLinearSystem(spline.assembleMatrix(mass), spline.assembleVector(b), self.yddot_old)

    # -- state
    @property
    def t(self):
        """time of the state ``y``, ``ydot``, ``yddot``"""
        return self.integrator.t - self.DELTA_T

    @property
    def t_alpha(self):
        return self.dyn.t_alpha

    @property
    def y(self):
        return self.y_old

    @property
    def ydot(self):
        return self.ydot_old

    @property
    def yddot(self):
        return self.yddot_old

    def energy(self):
        """``dyn.energy`` at the state of time ``t``: {"strain", "kinetic", "contact", "total"}"""
        return self.dyn.energy(self.spline.V, y=self.y_old, ydot=self.ydot_old)

    # -- stepping
    def _predict(self):
        it = self.integrator
        if self.scheme == "generalized_alpha":
            it.sameVelocityPredictor().evaluate(out=self._y)
        else:
            LinearCombination([(1.0, self.y_old), (self.DELTA_T, self.ydot_old)]).evaluate(out=self._y)
        if hasattr(self._y, "invalidate_ghosts"):
            self._y.invalidate_ghosts()

    def step(self, n=1):
        """advances the state by ``n`` steps of ``DELTA_T``"""
        spline, dyn = self.spline, self.dyn
        for _ in range(int(n)):
            self._predict()
            seconds = {"assembly": 0.0, "solve": 0.0} if self.timing else None
            history = spline.solveNonlinearVariationalProblem(dyn, self._tangent, self._y, absoluteTolerance=self.absoluteTolerance,
                                                              phaseSeconds=seconds)
            active = dyn.active_points()
            self.integrator.advance()
            self.last = {"newton": history, "iterations": len(history) - 1, "active_points": active,
                         "assembly_seconds": seconds["assembly"] if self.timing else None,
                         "solve_seconds": seconds["solve"] if self.timing else None}
            self.steps_done += 1
        return self


class _FlowStep(object):
    """Residual and tangent of one time step of ``FlowTransientProblem`` as forms of the unknown x of level n+1: the flow law is
    read at the alpha-level state x_alpha (kept in a Function of its own) with the acceleration xdot_alpha = c_a x_alpha + a0,
    and R / alpha_f and (dR/dx) / alpha_f = K(x_alpha) are handed out -- the scaling of ``forms.DynamicResidual``."""

    def __init__(self, problem):
        self.problem, self.geometry, self.symmetric = problem, problem.inner.geometry, False

    def assemble_vector(self, V, row0=None, row1=None):
        pb = self.problem
        pb._read_state(V)
        r = pb.inner.assemble_vector(V, row0, row1)
        if pb.alpha_f != 1.0:
            _dev.vec_lincomb(r, [1.0 / pb.alpha_f], [r])
        return r

    def tangent(self):
        return self

    def assemble_matrix(self, V, row0=None, row1=None):
        self.problem._read_state(V)
        return self.problem.inner.tangent().assemble_matrix(V, row0, row1)

    def assemble_block(self, V, i, j, row0=None, row1=None):
        self.problem._read_state(V)
        return self.problem.inner.tangent().assemble_block(V, i, j, row0, row1)


class FlowTransientProblem(object):
    """Transient incompressible flow on an ``ExtractedSpline``: the first-order system of ``forms.FlowResidual`` in the state
    x = (u_1 .. u_nsd, p) by the generalized-alpha method for first-order systems (Jansen, Whiting & Hulbert 2000;
    ``scheme="generalized_alpha"``, ``RHO_INF``) or backward Euler (``scheme="backward_euler"``), one
    ``spline.solveNonlinearVariationalProblem`` per step.  ``flow``: the ``FlowResidual``; its ``u`` is the unknown x of the step
    being computed.

    The law is read at the ALPHA LEVEL, the WHOLE state including the pressure: x_alpha = alpha_f x + (1 - alpha_f) x_old, with
    the acceleration xdot_alpha = alpha_m xdot + (1 - alpha_m) xdot_old of the velocity fields (the pressure has no rate in
    the equations: c_a acts on the velocity fields only).  The pressure of the state is therefore the one that makes
    x_alpha satisfy the equations, extrapolated to level n+1; for backward Euler the levels coincide.  From the integrator's
    ``xdot_alpha().split(x)`` = (c, rest):  c_a = d xdot_alpha / d x_alpha = c / alpha_f  and  a0 = rest - c_a (1 - alpha_f) x_old,
    a nodal vector taken to the points field by field; tau_M takes 4 / DELTA_T^2.  The Newton solve sees R / alpha_f and
    (dR/dx) / alpha_f, as ``forms.DynamicResidual`` scales them.

    ``x0`` / ``xdot0``: FE Functions, IGA-dof ``DeviceVector`` s (prolonged by M) or None = 0; ``xdot0`` should be compatible
    with the equations (generalized-alpha over-determines the start).  ``step(n)``; ``x``, ``xdot``: the state at time ``t``;
    ``last``: {"newton": relative norms, "iterations"} of the last step.  With ``absoluteTolerance`` > 0 a step also ends,
    without a Newton step, when the first residual norm is at most that."""

    def __init__(self, spline, flow, DELTA_T, scheme="generalized_alpha", RHO_INF=0.5, x0=None, xdot0=None, t=0.0,
                 absoluteTolerance=0.0):
        from . import forms as _forms
        from .common import Function
        who = "FlowTransientProblem"
        if scheme not in ("generalized_alpha", "backward_euler"):
            raise ValueError("%s: scheme must be 'generalized_alpha' or 'backward_euler', not %r" % (who, scheme))
        if DELTA_T is None or not float(DELTA_T) > 0.0:
            raise ValueError("%s: DELTA_T must be positive, not %r" % (who, DELTA_T))
        if scheme == "generalized_alpha" and not 0.0 <= float(RHO_INF) <= 1.0:
            raise ValueError("%s: RHO_INF must lie in [0, 1], not %r" % (who, RHO_INF))
        if not float(absoluteTolerance) >= 0.0:
            raise ValueError("%s: absoluteTolerance = %r must not be negative" % (who, absoluteTolerance))
        if spline._distributed():
            raise NotImplementedError("%s: several ranks are not supported" % who)
        if spline._caller_ordered():
            raise NotImplementedError("%s: a spline with the caller's FE dof order (feOrder) is not supported" % who)
        if not isinstance(flow, _forms.FlowResidual):
            raise NotImplementedError("%s: flow = %r; a FlowResidual carries the law" % (who, flow))
        self.spline, self.flow, self.scheme = spline, flow, scheme
        self.DELTA_T, self.absoluteTolerance = float(DELTA_T), float(absoluteTolerance)
        self._x = flow.u
        V = spline.V
        self.x_old, self.xdot_old, self._x_alpha = Function(V), Function(V), Function(V)
        self._set_initial(self.x_old, x0)
        self._set_initial(self.xdot_old, xdot0)
        if scheme == "generalized_alpha":
            self.integrator = GeneralizedAlphaIntegrator(float(RHO_INF), self.DELTA_T, self._x, [self.x_old, self.xdot_old], t=float(t))
            self.alpha_f = self.integrator.ALPHA_F
            rate = self.integrator.xdot_alpha()
        else:
            self.integrator = BackwardEulerIntegrator(self.DELTA_T, self._x, [self.x_old], t=float(t))
            self.alpha_f = 1.0
            rate = self.integrator.xdot()
        c, rest = rate.split(self._x)
        self.c_a = c / self.alpha_f
        self._a0 = rest - self.c_a * (1.0 - self.alpha_f) * LinearCombination.of(self.x_old)
        self._state = x_alpha(self.alpha_f, self._x, self.x_old)
        _vec_of(self._x)[:] = _vec_of(self.x_old)
        self.inner = flow._at(self._x_alpha)
        self.inner.c_a, self.inner.dt4 = self.c_a, 4.0 / self.DELTA_T ** 2
        self._a0_nodal = DeviceVector(_vec_of(self._x).size(), zero=False)
        self._form = _FlowStep(self)
        self.last = None
        self.steps_done = 0

    def _set_initial(self, f, v):
        _set_initial_state("FlowTransientProblem", self.spline, f, v)

    def _read_state(self, V):
        """x_alpha into the Function the law reads; a0 of the velocity fields at the points once per step: it depends on the
        old state only (``step`` and ``advance`` mark it stale)"""
        inner = self.inner
        self._state.evaluate(out=self._x_alpha)
        if inner.a0 is not None:
            return
        self._a0.evaluate(out=self._a0_nodal)
        g, nF, pts = inner._scope(V, "FlowTransientProblem")
        nsd, n = pts.nsd, g.num_nodes()
        a0 = DeviceVector(nsd * pts.npts, zero=False)
        ui = DeviceVector(n, zero=False)
        for i in range(nsd):
            _dev.vec_copy_range(ui, 0, self._a0_nodal, i * n, n)
            _dev.vec_copy_range(a0, i * pts.npts, _dev.quad_eval(pts.verts, pts.p, pts.cp, ui, nq=pts.nq, rational=inner.rational), 0, pts.npts)
        inner.a0 = a0

    @property
    def t(self):
        """time of the state ``x``, ``xdot``"""
        return self.integrator.t - self.DELTA_T

    @property
    def x(self):
        return self.x_old

    @property
    def xdot(self):
        return self.xdot_old

    def step(self, n=1):
        """advances the state by ``n`` steps of ``DELTA_T`` (the predictor is the old state)"""
        spline = self.spline
        for _ in range(int(n)):
            _vec_of(self._x)[:] = _vec_of(self.x_old)
            if hasattr(self._x, "invalidate_ghosts"):
                self._x.invalidate_ghosts()
            self.inner.a0 = None                                         # (the old state is new: a0 is formed at the first assembly)
            history = spline.solveNonlinearVariationalProblem(self._form, self._form, self._x, absoluteTolerance=self.absoluteTolerance)
            if self.scheme == "backward_euler":
                self.integrator.xdot().evaluate(out=self.xdot_old)       # (the state keeps a rate for either scheme)
            self.integrator.advance()
            self.inner.a0 = None
            self.last = {"newton": history, "iterations": len(history) - 1}
            self.steps_done += 1
        return self
