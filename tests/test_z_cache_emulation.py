"""CPU: the z walk of the tensor-pattern PtAP that holds the last B2 block of every node slot in registers
(tigar_amd/csrc/tg_tensor_body.h: tt_z_lane<P, true>), executed lane by lane by a host build of the header
(tests/emu/z_cache_emu.cpp).  The reference K comes from the plain walk tt_z_lane<P> on a table of distinct pointers
whose class-equal planes hold copies of the same data; the holding walk runs on tables in which those planes share a
block.  Indices and values of K must agree bit for bit, for every class pattern, every split of the dof planes into
sub-slabs (warm-up elements before ka, seams), planes handed over in pieces, equal data behind different pointers, with
and without the zero-dof mask.  The device build of the same code is covered by tests/test_gpu_z_cache.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "z_cache_emu.cpp")
HDR = os.path.join(HERE, "..", "tigar_amd", "csrc", "tg_tensor_body.h")
c_f64p, c_i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _fresh(out):
    return os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def emu():
    build = os.path.join(HERE, "emu", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libz_cache_emu.so")
    if not _fresh(so):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", SRC, "-o", so])
    lib = C.CDLL(so)
    lib.emu_z_repeats.restype = C.c_int
    lib.emu_z_block_loads.restype = C.c_int
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _kps(nel, p):
    ncp = nel + p
    kps = np.zeros(ncp + 1, dtype=np.int32)
    for i in range(ncp):
        kps[i + 1] = kps[i] + (min(ncp - 1, i + p) - max(0, i - p) + 1)
    return kps


def _rn(p, a, nfe):
    return 2 * p + 1 if (a % p == 0 and 0 < a < nfe - 1) else p + 1


def _uniform_class(p, a, nfe):
    """first plane, last plane, the p - 1 nodes inside an element, the vertices between two elements"""
    if a == 0:
        return "first"
    if a == nfe - 1:
        return "last"
    return "vertex" if a % p == 0 else "node%d" % (a % p)


def _patterns(p, nel2):
    """name -> (data class, block) per FE plane: planes of one data class hold equal data, planes with the same block key
    share ONE block in the table the holding walk reads (the block key refines the data class)"""
    nfe = p * nel2 + 1
    uni = [_uniform_class(p, a, nfe) for a in range(nfe)]
    own = list(range(nfe))
    half = nfe // 2
    pats = {
        "uniform": (uni, uni),
        "distinct": (own, own),
        "uniform-then-distinct": ([uni[a] if a < half else a for a in range(nfe)],) * 2,
        "distinct-then-uniform": ([a if a < half else uni[a] for a in range(nfe)],) * 2,
        # the planes reach the stage in two pieces of the ring: same classes, other blocks behind the seam
        "uniform-two-pieces": (uni, [(uni[a], a < half) for a in range(nfe)]),
        "uniform-single-plane-pieces": (uni, [(uni[a], a) for a in range(nfe)]),
        # a plane and its successor at stride p: equal data, different pointers (every second element keeps copies)
        "equal-data-other-pointer": (uni, [(uni[a], a if ((a - 1) // p) % 2 else -1) for a in range(nfe)]),
    }
    return pats


def _case(p, nel2, seed):
    W, Q = 2 * p + 1, p + 1
    ncp0, ncp1, ncp2, nfe = p + 2, p + 1, nel2 + p, p * nel2 + 1
    rng = np.random.default_rng(seed)
    kps = [_kps(2, p), _kps(1, p), _kps(nel2, p)]
    wl = np.ascontiguousarray(rng.standard_normal((nel2, Q, Q)))
    mask = (rng.random(ncp0 * ncp1 * ncp2) < 0.3).astype(np.uint8)
    return dict(p=p, nel2=nel2, W=W, ncp=(ncp0, ncp1, ncp2), nfe=nfe, kps=kps, wl=wl, mask=mask, rng=rng)


def _blocks(cs, data_cls, block_key):
    """(reference pointers, shared pointers, arrays to keep alive)"""
    p, W, nfe, (ncp0, ncp1, _) = cs["p"], cs["W"], cs["nfe"], cs["ncp"]
    data, shared, keep, pref, pali = {}, {}, [], [], []
    for a in range(nfe):
        n = W * W * _rn(p, a, nfe) * ncp0 * ncp1
        if data_cls[a] not in data:
            data[data_cls[a]] = cs["rng"].standard_normal(n)
        d = data[data_cls[a]]
        assert d.size == n                                   # (planes of one class have one block length)
        mine = d.copy()
        keep.append(mine)
        pref.append(mine.ctypes.data)
        if block_key[a] not in shared:
            shared[block_key[a]] = d.copy()
        pali.append(shared[block_key[a]].ctypes.data)
    assert len(set(pref)) == nfe
    return pref, pali, keep + list(shared.values())


def _run(emu, cs, ptrs, held, splits, masked):
    p, nel2, W, (ncp0, ncp1, ncp2), kps = cs["p"], cs["nel2"], cs["W"], cs["ncp"], cs["kps"]
    w01 = int(kps[0][ncp0]) * int(kps[1][ncp1])
    nnz = w01 * int(kps[2][ncp2])
    kcol, kval = np.full(nnz, -1, dtype=np.int32), np.full(nnz, np.nan)
    at, loads = 0, []
    for ka, kb in splits:
        e_begin, e_end = max(0, ka - p), min(nel2, kb)
        plo, phi = (0 if e_begin == 0 else p * e_begin + 1), p * e_end
        tab = (C.c_void_p * (phi - plo + 1))(*ptrs[plo:phi + 1])
        emu.emu_zc(int(held), p, tab, plo, nel2, _p(cs["wl"], c_f64p), _p(kps[2], c_i32p), ncp0, ncp1, _p(kps[0], c_i32p),
                   _p(kps[1], c_i32p), ka, kb, max(1, 64 // (W * W)), C.cast(kcol.ctypes.data + 4 * at, c_i32p),
                   C.cast(kval.ctypes.data + 8 * at, c_f64p), _p(cs["mask"], C.POINTER(C.c_uint8)) if masked else None,
                   C.c_double(2.5))
        at += w01 * int(kps[2][kb] - kps[2][ka])
        loads.append((emu.emu_z_repeats(p, tab, len(tab)), len(tab),
                      emu.emu_z_block_loads(p, plo, cs["nfe"], tab, len(tab), int(held))))
    assert at == nnz and np.all(kcol >= 0) and not np.any(np.isnan(kval))      # every slot of K written
    return kcol, kval, loads


def _splits(ncp2):
    yield [(0, ncp2)]
    for cut in range(1, ncp2):
        yield [(0, cut), (cut, ncp2)]
    yield [(i, i + 1) for i in range(ncp2)]


@pytest.mark.parametrize("nel2", [1, 2, 5, 8])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_holding_walk_is_bit_identical_to_the_plain_walk_on_copies(emu, p, nel2):
    cs = _case(p, nel2, seed=11 * p + nel2)
    ncp2 = cs["ncp"][2]
    for name, (data_cls, block_key) in _patterns(p, nel2).items():
        pref, pali, _keep = _blocks(cs, data_cls, block_key)
        for masked in (False, True):
            ref = {}
            for splits in _splits(ncp2):
                # (the plain walk's K does not depend on the split either: one reference per mask, checked for each)
                c0, v0, _ = _run(emu, cs, pref, False, splits, masked)
                if not ref:
                    ref["c"], ref["v"] = c0, v0
                assert c0.tobytes() == ref["c"].tobytes() and v0.tobytes() == ref["v"].tobytes(), (name, splits)
                c1, v1, _ = _run(emu, cs, pali, True, splits, masked)
                assert c1.tobytes() == c0.tobytes() and v1.tobytes() == v0.tobytes(), (name, masked, splits)
                # holding on a table without repeats, and not holding on one with: the same K again
                c2, v2, _ = _run(emu, cs, pref, True, splits, masked)
                c3, v3, _ = _run(emu, cs, pali, False, splits, masked)
                assert c2.tobytes() == c0.tobytes() and v2.tobytes() == v0.tobytes(), (name, masked, splits)
                assert c3.tobytes() == c0.tobytes() and v3.tobytes() == v0.tobytes(), (name, masked, splits)


@pytest.mark.parametrize("p", [1, 2, 3])
def test_host_side_choice_and_load_count(emu, p):
    """what tg_tensor_zstage decides and counts from the pointer table: a table repeats at stride p exactly when two
    planes p apart share a block; the holding walk loads one block per change of pointer in a slot, the two ends of the
    grid always, the plain walk one per plane"""
    for nel2 in (1, 2, 5, 8):
        cs = _case(p, nel2, seed=3)
        nfe, ncp2 = cs["nfe"], cs["ncp"][2]
        pats = _patterns(p, nel2)
        whole = [(0, ncp2)]
        _, pali, _k = _blocks(cs, *pats["uniform"])
        rep, n, loads = _run(emu, cs, pali, True, whole, False)[2][0]
        assert n == nfe and _run(emu, cs, pali, False, whole, False)[2][0][2] == nfe
        if nel2 >= 3:
            assert rep == 1
        # node 0, the last node, the p - 1 nodes inside an element and (two elements or more) the vertices: one block each,
        # however many elements
        assert loads == 2 + (p - 1) + (1 if nel2 >= 2 else 0)
        _, pown, _k = _blocks(cs, *pats["distinct"])
        rep, n, loads = _run(emu, cs, pown, True, whole, False)[2][0]
        assert rep == 0 and loads == n == nfe
        _, peq, _k = _blocks(cs, *pats["equal-data-other-pointer"])
        loads_eq = _run(emu, cs, peq, True, whole, False)[2][0][2]
        assert loads_eq == nfe                       # every element another pointer in every slot: all reload
        _, psingle, _k = _blocks(cs, *pats["uniform-single-plane-pieces"])
        assert _run(emu, cs, psingle, True, whole, False)[2][0][::2] == (0, nfe)


def test_stand_alone_program_under_the_host_sanitizers():
    """the same header as a program with its own main (its own cases: plain walk on copies against the holding walk on
    shared blocks), built with AddressSanitizer and UndefinedBehaviorSanitizer: no report, every K equal"""
    build = os.path.join(HERE, "emu", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "z_cache_emu_san")
    if not _fresh(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DZ_CACHE_EMU_MAIN", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-2000:]
