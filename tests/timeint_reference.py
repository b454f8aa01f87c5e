"""Plain dense reference of the time integrators (tigar_amd/timeIntegration.py), for the tests: generalized-alpha and
backward Euler for

    order 2:  M a + C v + K x = f(t),  C = a_M M + a_K K        order 1:  M v + K x = f(t)

on given dense K, M, damping and load, in any numpy float type (numpy.longdouble as the reference proper, float64 for
numpy's own rounding error).  The recurrences are written in the RATE form of the literature -- the unknown of a step is
the new acceleration (order 2: Newmark's x1 = x0 + dt v0 + dt^2 ((1/2 - beta) a0 + beta a1), v1 = v0 + dt ((1 - gamma) a0 +
gamma a1), balance at the alpha levels, Chung & Hulbert 1993) or the new velocity (order 1, Jansen, Whiting & Hulbert
2000) -- not in the displacement form the package solves, so the two share no formula.  The effective matrix is factorised
once by a Cholesky factorisation written here, in the working precision.  No fixtures here (like fd_reference.py): a
module the tests import."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def parameters(rho_inf, order, first_order_alpha_m=False):
    """(alpha_m, alpha_f, gamma, beta) in closed form"""
    rho = float(rho_inf)
    if order == 1 or first_order_alpha_m:
        am = (3.0 - rho) / (2.0 * (1.0 + rho))
    else:
        am = (2.0 - rho) / (1.0 + rho)
    af = 1.0 / (1.0 + rho)
    gamma = 0.5 + am - af
    beta = 0.25 * (1.0 + am - af) ** 2
    return am, af, gamma, beta


def cholesky(A):
    """lower factor L of a symmetric positive definite A, in A's dtype (column by column)"""
    A = np.array(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def cho_solve(L, b):
    n = L.shape[0]
    y = np.zeros(n, dtype=L.dtype)
    for i in range(n):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(n, dtype=L.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def energy(K, M, x, v):
    return 0.5 * float(v @ (M @ v)) + 0.5 * float(x @ (K @ x))


def integrate(K, M, dt, steps, order=2, scheme="generalized_alpha", rho_inf=0.5, damping=None, load=None, x0=None, v0=None,
              t0=0.0, dtype=np.float64, first_order_alpha_m=False):
    """Returns {"t": [t_0 .. t_steps], "x": [...], "v": [...], "a": [...]} (lists of vectors of ``dtype``; "a" only for order
    2, "v" not for backward Euler of order 1).  ``load``: None or ``t -> vector``.  ``x0`` / ``v0``: None = 0.  The initial
    acceleration of order 2 (generalized-alpha) is the compatible one, M a0 = f(t0) - C v0 - K x0; so is the initial velocity
    of a first-order generalized-alpha problem when ``v0`` is None."""
    T = dtype
    K = np.asarray(K, dtype=T)
    M = np.asarray(M, dtype=T)
    n = K.shape[0]
    dt = T(dt)
    aM, aK = (T(0), T(0)) if damping is None else (T(damping[0]), T(damping[1]))
    C = aM * M + aK * K

    def f(t):
        return np.zeros(n, dtype=T) if load is None else np.asarray(load(float(t)), dtype=T)

    x = np.zeros(n, dtype=T) if x0 is None else np.asarray(x0, dtype=T)
    given_v0 = v0 is not None
    v = np.zeros(n, dtype=T) if v0 is None else np.asarray(v0, dtype=T)
    out = {"t": [float(t0)], "x": [x.copy()]}
    gen_alpha = scheme == "generalized_alpha"
    if not gen_alpha and scheme != "backward_euler":
        raise ValueError(scheme)
    half, one = T(1) / T(2), T(1)

    if gen_alpha:
        am, af, gamma, beta = (T(c) for c in parameters(rho_inf, order, first_order_alpha_m))
        LM = cholesky(M)
        if order == 2:
            a = cho_solve(LM, f(t0) - C @ v - K @ x)
            out["v"], out["a"] = [v.copy()], [a.copy()]
            L = cholesky(am * M + (af * gamma * dt) * C + (af * beta * dt * dt) * K)
            for s in range(steps):
                t_new = t0 + (s + 1) * float(dt)
                t_alpha = t_new - (1.0 - float(af)) * float(dt)
                xp = x + af * (dt * v + (dt * dt * (half - beta)) * a)      # x at the alpha level without a1
                vp = v + (af * dt * (one - gamma)) * a                     # v at the alpha level without a1
                a1 = cho_solve(L, f(t_alpha) - M @ ((one - am) * a) - C @ vp - K @ xp)
                x = x + dt * v + (dt * dt) * ((half - beta) * a + beta * a1)
                v = v + dt * ((one - gamma) * a + gamma * a1)
                a = a1
                out["t"].append(t_new)
                out["x"].append(x.copy())
                out["v"].append(v.copy())
                out["a"].append(a.copy())
        else:
            if not given_v0:
                v = cho_solve(LM, f(t0) - K @ x)
            out["v"] = [v.copy()]
            L = cholesky(am * M + (af * gamma * dt) * K)
            for s in range(steps):
                t_new = t0 + (s + 1) * float(dt)
                t_alpha = t_new - (1.0 - float(af)) * float(dt)
                xp = x + (af * dt * (one - gamma)) * v
                v1 = cho_solve(L, f(t_alpha) - M @ ((one - am) * v) - K @ xp)
                x = x + dt * ((one - gamma) * v + gamma * v1)
                v = v1
                out["t"].append(t_new)
                out["x"].append(x.copy())
                out["v"].append(v.copy())
    else:
        if order == 2:
            out["v"] = [v.copy()]
            # unknown: the new velocity; x1 = x0 + dt v1, a1 = (v1 - v0) / dt
            L = cholesky(M / dt + C + dt * K)
            for s in range(steps):
                t_new = t0 + (s + 1) * float(dt)
                v1 = cho_solve(L, f(t_new) + M @ (v / dt) - K @ x)
                x = x + dt * v1
                v = v1
                out["t"].append(t_new)
                out["x"].append(x.copy())
                out["v"].append(v.copy())
        else:
            L = cholesky(M / dt + K)
            for s in range(steps):
                t_new = t0 + (s + 1) * float(dt)
                x = cho_solve(L, f(t_new) + M @ (x / dt))
                out["t"].append(t_new)
                out["x"].append(x.copy())
    return out


def fe_pair_1d(n):
    """(K, M) of linear finite elements on n + 1 equal cells of (0, 1) with both ends clamped: n unknowns, dense"""
    h = 1.0 / (n + 1)
    K = (np.diag(np.full(n, 2.0)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)) / h
    M = (np.diag(np.full(n, 4.0)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)) * (h / 6.0)
    return K, M
