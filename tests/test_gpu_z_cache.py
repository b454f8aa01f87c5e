"""-m gpu: the z pass of the tensor-pattern PtAP over planes that share B2 blocks (one FE plane contracted per class,
tests/test_gpu_plane_classes.py) holds the last block of every node slot of an element in registers and loads a block
only when the pointer of its slot changes (k_tt_z_held, csrc/tg_tensor_body.h: tt_z_held).  K must be byte for byte
(indptr, indices, data) what the plain walk writes (TIGAR_TT_Z_CACHE=0) and what it is when every plane is contracted
(TIGAR_TT_PLANE_CLASSES=0: no pointer repeats, the plain kernel); tg_tensor_zstage_info shows which walk ran and how
many blocks a lane loaded."""
import pytest

pytestmark = pytest.mark.gpu

ENV = ("TIGAR_TT_PLANE_CLASSES", "TIGAR_TT_Z_CACHE", "TIGAR_IMPLICIT_M", "TIGAR_SUB_PLANES")


def _open_knots(p, verts):
    return [verts[0]] * p + list(verts) + [verts[-1]] * p


def _z_vertices(kind, n):
    """n elements on [0, 1] (all values exact in binary): uniform; graded (lengths (2 i + 1) / n^2, all different);
    uniform on the first half and graded on the second"""
    if kind == "uniform":
        return [float(i) / n for i in range(n + 1)]
    if kind == "graded":
        return [float(i * i) / (n * n) for i in range(n + 1)]
    h = n // 2
    return [float(i) / n for i in range(h)] + [0.5 + 0.5 * float(i * i) / (h * h) for i in range(h + 1)]


def _spline(p, nels, zkind):
    import tigar_amd as t
    from tigar_amd import BSplines as B
    kvs = [B.uniformKnots(p, 0., 1., nels[0]), B.uniformKnots(p, 0., 1., nels[1]), _open_knots(p, _z_vertices(zkind, nels[2]))]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * 3, kvs))
    sp0 = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))       # zero dofs on all faces
    return gen, t.ExtractedSpline(gen, 2 * p)


def _same_bytes(Ka, Kb):
    return Ka.indptr.tobytes() == Kb.indptr.tobytes() and Ka.indices.tobytes() == Kb.indices.tobytes() and \
        Ka.data.tobytes() == Kb.data.tobytes()


@pytest.fixture
def stages(monkeypatch):
    """(ka, kb, held, planes walked, block loads per lane) of every z stage run while the fixture lives"""
    from tigar_amd.tensorptap import TensorPtAP
    calls = []
    inner = TensorPtAP.zstage

    def spy(self, pieces, ka, kb, *args, **kwargs):
        out = inner(self, pieces, ka, kb, *args, **kwargs)
        calls.append((int(ka), int(kb)) + self.zstage_info())
        return out
    monkeypatch.setattr(TensorPtAP, "zstage", spy)
    return calls


def _assemble(p, nels, zkind, form, sub_planes, env):
    """K with TIGAR_IMPLICIT_M=1, sub-slabs of ``sub_planes`` dof planes and the settings ``env``; whatever the caller's
    environment held in these variables is put back"""
    with pytest.MonkeyPatch.context() as mp:
        for k in ENV:
            mp.delenv(k, raising=False)
        mp.setenv("TIGAR_IMPLICIT_M", "1")
        mp.setenv("TIGAR_SUB_PLANES", str(sub_planes))
        for k, v in env.items():
            mp.setenv(k, v)
        gen, spline = _spline(p, nels, zkind)
        K = spline.assembleMatrix(form, diag=2.0)
        assert getattr(gen.M, "is_implicit", False)
        return K.to_scipy()


def _three_ways(p, nels, zkind, form, sub, stages):
    """K with the default settings, with the plain z walk, with every plane contracted -- and the stages of each"""
    out = []
    for env in ({}, {"TIGAR_TT_Z_CACHE": "0"}, {"TIGAR_TT_PLANE_CLASSES": "0"}):
        del stages[:]
        out.append((_assemble(p, nels, zkind, form, sub, env), list(stages)))
    (K, st), (K_plain, st_plain), (K_all, st_all) = out
    assert _same_bytes(K, K_plain) and _same_bytes(K, K_all)
    ncp2 = nels[2] + p
    for s in (st, st_plain, st_all):
        assert s and s[0][0] == 0 and s[-1][1] == ncp2 and all(a[1] == b[0] for a, b in zip(s, s[1:]))    # every dof plane once
    # the plain walk loads one block per plane; so does every stage when no two planes share a block
    assert all(not held and loads == planes for _, _, held, planes, loads in st_plain + st_all)
    assert [s[:2] + s[3:4] for s in st_plain] == [s[:2] + s[3:4] for s in st]
    return st


@pytest.mark.parametrize("zkind", ["uniform", "graded", "half"])
@pytest.mark.parametrize("p,nels", [(3, (5, 4, 8)), (2, (6, 5, 8)), (1, (4, 4, 8))])
def test_K_is_byte_for_byte_that_of_the_plain_walk(p, nels, zkind, stages):
    """LaplaceForm (three terms) and MassForm (one), zero dofs on all faces, in sub-slabs of 2 and 3 dof planes (stages
    that begin with warm-up elements, planes handed over by the ring: other pointers for the same class) and in one"""
    from tigar_amd import forms as F
    nfe2 = p * nels[2] + 1
    for form in (F.LaplaceForm(), F.MassForm()):
        for sub in (2, 3, 64):
            st = _three_ways(p, nels, zkind, form, sub, stages)
            assert all(loads == planes for _, _, held, planes, loads in st if not held)
            assert all(loads <= planes for _, _, held, planes, loads in st if held)
            if zkind == "graded":
                assert not any(held for _, _, held, _, _ in st)               # every plane its own block: the plain kernel
            if sub == 64:
                assert [s[:2] for s in st] == [(0, nels[2] + p)] and st[0][3] == nfe2
                held, loads = st[0][2], st[0][4]
                if zkind == "uniform":
                    # first plane, last plane, the p - 1 nodes inside an element, the vertices: one block each
                    assert held and loads == p + 2
                elif zkind == "half":
                    assert held and p + 2 < loads < nfe2
            elif zkind == "uniform" and p > 1:
                # (p = 1 is asserted in one sub-slab above: whether a short stage sees two vertex planes of ONE piece of the
                #  ring depends on where the pieces end)
                assert any(held and loads < planes for _, _, held, planes, loads in st)


@pytest.mark.parametrize("p,nels", [(3, (5, 4, 1)), (2, (6, 5, 2))])
def test_one_and_two_elements_along_z(p, nels, stages):
    """nel2 = 1: the opening vertex, the nodes inside and the last node only, nothing to hold; nel2 = 2: one shared
    vertex, nodes inside the two elements p planes apart"""
    from tigar_amd import forms as F
    st = _three_ways(p, nels, "uniform", F.LaplaceForm(), 64, stages)
    nfe2 = p * nels[2] + 1
    assert len(st) == 1 and st[0][3] == nfe2
    if nels[2] == 1:
        assert not st[0][2] and st[0][4] == nfe2
    else:
        assert st[0][2] and st[0][4] == p + 2


def test_block_loads_do_not_grow_with_the_number_of_elements(stages):
    from tigar_amd import forms as F
    p = 3
    loads = []
    for nel2 in (4, 8):
        del stages[:]
        _assemble(p, (5, 4, nel2), "uniform", F.LaplaceForm(), 64, {})
        assert len(stages) == 1 and stages[0][2] and stages[0][3] == p * nel2 + 1
        loads.append(stages[0][4])
    assert loads == [p + 2, p + 2]


def test_pair_plans_of_different_bases():
    """K_fg = M_f^T A M_g for the components of a div-conforming B-spline (degrees (1, 1, 1), elements (1, 1, 2); all
    fields extract to one Q_2 grid) through plan.zstage: the nodes inside the two elements share a block"""
    from tigar_amd import BSplines as B, common as tc, device as dev, forms as F
    from tigar_amd.compatibleSplines import BSplineCompat
    from tigar_amd.kronptap import KronExtraction
    from tigar_amd.tensorptap import TensorPtAP
    dev.device_info()
    degs, nels = (1, 1, 1), (1, 1, 2)
    kv = [B.uniformKnots(degs[k], 0., 1. + 0.25 * k, nels[k]) for k in range(3)]
    gen = BSplineCompat(tc.selfcomm, B.ExplicitBSplineControlMesh(list(degs), kv), "RT", list(degs))
    kxs = [KronExtraction(gen.getFieldSpline(f), gen.V.grids[f]) for f in range(3)]
    g = gen.V.grids[0]
    V1 = type(gen.V)([g], gen.V.element)
    factors = F.LaplaceForm().factors(V1)
    nz = g.shape()[-1]
    for f in range(3):
        for gg in range(3):
            plan = TensorPtAP.for_pair(kxs[f], kxs[gg])
            assert plan is not None
            packed = plan.pack_kron_factors(factors)
            assert packed is not None
            Ks, infos = [], []
            for env in ({}, {"TIGAR_TT_Z_CACHE": "0"}, {"TIGAR_TT_PLANE_CLASSES": "0"}):
                with pytest.MonkeyPatch.context() as mp:
                    for k in ("TIGAR_TT_PLANE_CLASSES", "TIGAR_TT_Z_CACHE"):
                        mp.delenv(k, raising=False)
                    for k, v in env.items():
                        mp.setenv(k, v)
                    piece = plan.planes_kron(packed, 0, nz)
                    assert piece is not None
                    Ks.append(plan.zstage([piece], 0, kxs[f].ncp[2]).to_scipy())
                    infos.append(plan.zstage_info())
            assert Ks[0].nnz == plan.k_nnz(0, kxs[f].ncp[2]) and _same_bytes(Ks[0], Ks[1]) and _same_bytes(Ks[0], Ks[2])
            assert infos[0][0] and infos[0][1] == nz and infos[0][2] < nz
            assert infos[1] == (False, nz, nz) and infos[2] == (False, nz, nz)
