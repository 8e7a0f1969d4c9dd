"""CPU: the host side of the two-point Brownian query (``BrownianTreeNoiseSampler.pair`` -> ``sonar_brownian_pair_f32``) -- the split of two
points' expansions into the shared and the two private term lists, the entry point's declaration / binding / export, and its refusals,
which come back before anything touches the HIP runtime."""
import ctypes as C
import importlib
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sonar_brownian_pair_f32"
T_LO, T_HI = 0.03, 14.6


def triples(depth, count=200):
    """Seeded (t, s, t') inside [T_LO, T_HI]; the first ones are the edge cases: s == t', a time at either end of the range, times within
    half a grid cell of each other (they resolve to one grid point or to neighbours)."""
    rng = random.Random(1000 + depth)
    cell = (T_HI - T_LO) / (1 << depth)
    out = [(9.0, 4.0, 4.0), (9.0, T_LO, 4.0), (9.0, 4.0, T_LO), (T_HI, 9.0, 4.0), (4.0, T_HI, 9.0), (4.0, 9.0, T_HI), (T_LO, 4.0, T_HI),
           (9.0, 4.0, 4.0 + 0.4 * cell), (9.0, 4.0 + 0.2 * cell, 4.0 - 0.2 * cell), (9.0, 4.0, 4.0 + 0.6 * cell), (9.0, T_LO + 0.3 * cell, T_LO)]
    while len(out) < count:
        t = rng.uniform(T_LO, T_HI)
        s = rng.uniform(T_LO, t)
        out.append((t, s, rng.uniform(T_LO, s) if rng.random() < 0.7 else s - rng.random() * cell))
    return out


@pytest.mark.parametrize("depth", [6, 12, 24])
def test_split_reassembles_both_expansions_exactly(pkg, depth):
    """shared + only_i IS point i's expansion -- the same nodes with the same fp64 coefficients, in ascending id order -- and the three lists
    together are never longer than the two expansions."""
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    path = ng.BrownianPath(T_LO, T_HI, depth)
    some_shared = 0
    for t, s, t2 in triples(depth):
        path.coefficients(t)
        c1, c2 = dict(path.coefficients(s)), dict(path.coefficients(t2))
        shared, only_1, only_2 = ng.BrownianPath.split_pair(c1, c2)
        for ids, coefs in (shared, only_1, only_2):
            assert list(ids) == sorted(set(ids)) and len(ids) == len(coefs)
        assert not set(shared[0]) & (set(only_1[0]) | set(only_2[0]))
        for c, only in ((c1, only_1), (c2, only_2)):
            again = dict(zip(shared[0], shared[1])) | dict(zip(only[0], only[1]))
            assert again == c and len(again) == len(shared[0]) + len(only[0])
        assert len(shared[0]) + len(only_1[0]) + len(only_2[0]) <= len(c1) + len(c2)
        if path.resolve(s) == path.resolve(t2):
            assert not only_1[0] and not only_2[0]  # one grid point: everything is shared
        some_shared += bool(shared[0])
    assert some_shared  # (at least the coinciding points)


def test_split_shares_what_extension_points_have_in_common(pkg):
    """Beyond the range a new point is the outermost one plus ONE fresh normal: every earlier node keeps its coefficient, so it is shared."""
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    path = ng.BrownianPath(T_LO, T_HI, 0)
    c1, c2 = dict(path.coefficients(20.0)), dict(path.coefficients(25.0))
    shared, only_1, only_2 = ng.BrownianPath.split_pair(c1, c2)
    assert set(shared[0]) == set(c1) and only_1 == ([], []) and len(only_2[0]) == 1


def test_entry_point_is_declared_bound_and_exported(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    decl = re.search(rf"\bint {NAME}\s*\(([^)]*)\)\s*;", text)
    assert decl is not None, f"{NAME} is not declared in include/sonar_hip.h"
    assert NAME in hl.SIGNATURES
    kinds = {"float": C.c_float, "int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = hl.SIGNATURES[NAME]
    assert restype is C.c_int and len(params) == len(argtypes)
    for p, a in zip(params, argtypes):
        typ = p.rsplit(" ", 1)[0]
        assert a is (C.c_void_p if "*" in typ else kinds[typ]), p
    assert hasattr(hl.load(), NAME), f"{NAME} is not exported by the built library"
    src = open(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "noise_brownian.hip")).read()
    assert int(re.search(r"kMaxBrownianNodes = (\d+)", src).group(1)) == hl.BROWNIAN_MAX_TERMS
    assert int(re.search(r"kBrownLongTerms = (\d+)", src).group(1)) == hl.BROWNIAN_LONG_TERMS


def test_refusals_come_back_without_a_device(pkg):
    """Every call below is refused by the argument checks or has an empty output: the pointers are never dereferenced, nothing is launched."""
    hl = pkg.hip_lib
    fn = getattr(hl.load(), NAME)
    text = open(os.path.join(ROOT, "include", "sonar_hip.h")).read()
    OK, ARG, UNSUPPORTED = (int(re.search(rf"#define SONAR_{k} \(?(-?\d+)", text).group(1)) for k in ("OK", "ERR_ARG", "ERR_UNSUPPORTED"))
    o1, o2, w1, w2, prev, ba, bb = (0x1000 * (i + 1) for i in range(7))
    ids = lambda *v: (C.c_uint64 * len(v))(*v)  # noqa: E731
    cfs = lambda *v: (C.c_float * len(v))(*v)  # noqa: E731

    def call(out_1=o1, out_2=o2, w_1=w1, w_2=w2, prev=prev, base_1=(ba, 0.5, bb, 0.5), base_2=(ba, 0.25, bb, 0.75), n=4096, offs=0, shared=(), p1=(17, 35),
             p2=(17, 34), seed=5, latent_seeds=None, latent_elems=4096, part_1=None, part_2=None):
        lists = []
        for nodes in (shared, p1, p2):
            lists += [ids(*nodes), cfs(*([0.5] * len(nodes))), len(nodes)]
        return fn(out_1, out_2, w_1, w_2, prev, 1.0, -1.0, *base_1, *base_2, n, offs, *lists, seed, latent_seeds, latent_elems, part_1, part_2, None)

    assert call(n=0) == OK and call(n=0, w_1=None, w_2=None, prev=None, p1=(), p2=()) == OK  # an empty output launches nothing
    assert call(out_1=None) == ARG and call(out_2=None) == ARG
    assert call(out_2=o1) == ARG and call(w_1=o1) == ARG and call(w_2=w1) == ARG and call(w_2=o2) == ARG
    assert call(prev=o1) == ARG and call(prev=w2) == ARG
    assert call(base_1=(o2, 0.5, bb, 0.5)) == ARG and call(base_2=(ba, 0.5, w1, 0.5)) == ARG
    assert call(n=-1) == ARG and call(n=1 << 31) == ARG and call(offs=-4) == ARG
    assert call(p1=(35, 17)) == ARG and call(p2=(17, 17)) == ARG and call(shared=(3, 2)) == ARG  # every list ascends strictly
    assert call(shared=(17,)) == ARG                                                             # shared and private lists are disjoint
    assert call(p1=(1 << 48,)) == ARG
    assert call(latent_seeds=0x9000, offs=2) == ARG and call(latent_seeds=0x9000, latent_elems=6) == ARG
    many = tuple(range(100, 100 + hl.BROWNIAN_MAX_TERMS // 2))
    assert call(n=0, p1=many, p2=many) == OK                                                     # 96 terms over the lists: allowed
    assert call(p1=many, p2=many, shared=(7,)) == UNSUPPORTED and call(n=0, p1=many + (999,), p2=many) == UNSUPPORTED
    # statistics with one expansion below the long-expansion length and one at it: the two single launches would differ in block size
    assert call(part_1=0xA000, part_2=0xB000, p1=(17,), p2=(17, 34, 68, 136)) == UNSUPPORTED
    assert b"sonar_brownian_pair_f32" in hl.load().sonar_last_error()


def test_standalone_validator_if_built():
    """tools/brownian_pair_validate.cpp built with the host sanitizers (DESIGN.md has the command) calls the same refusing paths."""
    exe = os.path.join(ROOT, "scratch", "bin", "brownian_pair_validate")
    if not os.path.exists(exe):
        pytest.skip("scratch/bin/brownian_pair_validate has not been built")
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and "0 unexpected return codes" in run.stdout, run.stdout + run.stderr
