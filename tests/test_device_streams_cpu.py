"""CPU: the numpy statement of the generate-mode streams (oracle/device_streams.py) against published known-answer vectors and plain
Python integers, the draw orders of the half-spectrum against the half-spectrum itself, and the host's Brownian expansion against an
independent evaluation of the virtual Brownian tree.  The GPU side (tests/test_gpu_generate_oracle.py) compares the kernels with it."""
import math
import random

import numpy as np
import pytest

from oracle import device_streams as ds


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10, scalar and broadcast over an array."""
    assert _hex(ds.philox4x32_10(*ctr, *key)) == want
    arr = ds.philox4x32_10(*(np.full(3, c, dtype=np.uint64) for c in ctr), *key)
    assert all(_hex(w[i] for w in arr) == want for i in range(3))


def test_philox_extra_rounds_continue_the_key_schedule():
    """The spectrum's edge stream: 12 rounds = 10 rounds, then 2 more with the key bumped 10 times."""
    c, k = (1, 2, 3, 4), (5, 6)
    w10 = ds.philox4x32(*c, *k, rounds=10)
    k10 = ((5 + 10 * 0x9E3779B9) & 0xFFFFFFFF, (6 + 10 * 0xBB67AE85) & 0xFFFFFFFF)
    two_more = [int(v) for v in ds.philox4x32(*w10, *k10, rounds=2)]
    assert [int(v) for v in ds.philox4x32(*c, *k, rounds=12)] == two_more


def test_hash_known_answers():
    assert ds.splitmix64(0) == 0xE220A8397B1DCDAF
    assert int(ds.fmix32(1)) == 0x514E28B7
    assert int(ds.fmix32(0)) == 0


def test_mwc_steps_against_python_integers():
    rnd = random.Random(3)
    for _ in range(50):
        a, b = rnd.getrandbits(32), rnd.getrandbits(32)
        g = ds.Mwc.seeded(a, b)
        x, c = a, (b >> 1) | 1
        assert 1 <= c < 2**31
        for _ in range(20):
            assert int(g.next()) == x ^ c
            t = ds.MWC_A * x + c
            x, c = t & 0xFFFFFFFF, t >> 32


def test_rng_stream_key_word_and_truncated_stream_bits():
    """The fourth counter word is ((stream >> 32) << 16) ^ lane truncated to 32 bits: bits 48..63 of a stream id do not reach it, bits 32..47
    do, and the lane is folded into the same word."""
    s = 0x0000_1234_89AB_CDEF

    def first_words(stream, lane):
        return [int(v) for v in ds.rng_stream(7, stream, 5, lane).words(4)]

    assert first_words(s, 3) == first_words(s | (0xBEEF << 48), 3)
    assert first_words(s, 3) != first_words(s ^ (1 << 32), 3)
    assert first_words(s, 3) != first_words(s, 2)
    w = ds.philox4x32_10(5, 0, s & 0xFFFFFFFF, (((s >> 32) << 16) & 0xFFFFFFFF) ^ 3, 7, 0)
    g = ds.Mwc.seeded(w[0] ^ w[2], w[1] ^ w[3])
    assert first_words(s, 3) == [int(v) for v in g.words(4)]


def test_tile_walk_maps_elements_to_words():
    """Element e is word 4 * step + slot of lane (e % 256) // 4's burst in tile e // 4096 -- stream_words states the walk through the
    bursts themselves; the two must agree for any window."""
    e = np.array([0, 1, 3, 4, 255, 256, 4095, 4096, 4097, 7 * 4096 + 2, 3 * 4096 + 4])
    tile, lane, step, slot = ds.tile_position(e)
    assert list(tile[-4:]) == [1, 1, 7, 3] and list(lane[:6]) == [0, 0, 0, 1, 63, 0] and step[6] == 15 and list(slot[:4]) == [0, 1, 3, 0]
    for seed, stream in ((0, 0), (2**32 + 5, 2**47 + 1), (2**64 - 1, 2**32 + 3)):
        words = ds.stream_words(seed, stream, 8 * 4096)
        for i in range(len(e)):
            g = ds.rng_stream(seed, stream, int(tile[i]), int(lane[i]))
            assert int(words[e[i]]) == int(g.words(64)[4 * step[i] + slot[i]])
        # a window at an offset is the same stream
        assert np.array_equal(ds.stream_words(seed, stream, 5000, 4093), words[4093:4093 + 5000])


def test_conversions_are_exact_in_fp32():
    w = np.array([0, 1, 0xFF, 0x100, 0x7FFFFFFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)
    for f in (ds.u01, ds.u01_open, ds.unit_mantissa_radius):
        v = f(w)
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert ds.u01(w).min() == 0.0 and ds.u01(w).max() < 1.0
    assert ds.u01_open(w).min() == 2.0**-25 and ds.u01_open(0x7FFFFFFF) == 0.5 - 2.0**-25
    assert ds.u01_open(0xFFFFFFFF) == 1.0 and ds.u01_open(0xFFFFFE00) == 1.0 - 2.0**-23  # fp32 ties to even
    u = ds.unit_mantissa_radius(w)
    assert u.max() == 1.0 and u.min() > 0.0 and ds.unit_mantissa_radius(0xFFFFFFFF) == 2.0**-23
    # angles: 16 bits each as fractions of a revolution -- the float the kernel builds is 128 + bits 0..22 / 2^16 (low half) or
    # 128 + bits 16..31 / 2^16 (high half), equal to these modulo whole revolutions
    t = np.array([0x12345678, 0xFFFF0000, 0x0000FFFF, 0x007FFFFF], dtype=np.uint64)
    lo_float = 128.0 + (t & np.uint64(0x7FFFFF)).astype(np.float64) * 2.0**-16
    hi_float = 128.0 + (t >> np.uint64(16)).astype(np.float64) * 2.0**-16
    assert np.array_equal(np.mod(lo_float, 1.0), ds.angle_lo(t)) and np.array_equal(np.mod(hi_float, 1.0), ds.angle_hi(t))
    assert ds.angle_lo(0x12345678) == 0x5678 / 65536 and ds.angle_hi(0x12345678) == 0x1234 / 65536


def test_normal_and_uniform_fills_are_windows_of_one_stream():
    seed, stream = 2**32 + 5, 2**32 + 3
    whole = ds.normal_fill(seed, stream, 4 * 4096 + 7)
    for off, n in ((0, 1), (1, 3), (4093, 4097), (7, 3 * 4096)):
        assert np.array_equal(ds.normal_fill(seed, stream, n, off), whole[off:off + n])
    z = ds.normal_fill(0, 0, 1 << 17)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    u = ds.uniform_fill(0, 0, 1 << 17)
    assert u.dtype == np.float32 and 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.01
    # Box-Muller pairs: slots 0 / 1 share a radius, as do 2 / 3
    g, w = whole[:4 * 4096].reshape(-1, 4), ds.stream_words(seed, stream, 4 * 4096).reshape(-1, 4)
    assert np.allclose(np.hypot(g[:, 0], g[:, 1]), np.sqrt(-2 * np.log(ds.u01_open(w[:, 0]))), rtol=1e-12)
    assert np.allclose(np.hypot(g[:, 2], g[:, 3]), np.sqrt(-2 * np.log(ds.u01_open(w[:, 2]))), rtol=1e-12)


def test_brownian_families_and_selector():
    assert ds.brownian_family(4 * 4096, 0, 4096) == "burst"
    assert ds.brownian_family(4 * 4096, 4096, 4096) == "burst"        # a shard on a latent boundary
    assert ds.brownian_family(4 * 4096, 2048, 4096) == "philox"       # not on a latent boundary
    assert ds.brownian_family(4 * 900, 0, 900) == "philox"            # latents not whole tiles
    assert ds.brownian_family(4 * 4096, 0, 4096, latent_seeds=[1, 2, 3, 4]) == "philox"
    # both are unit normals per node, independent across nodes
    for z in (ds.brownian_burst_z(11, [0, 1, 2**40 + 3], 4 * 4096), ds.brownian_philox_z(11, [0, 1, 2**40 + 3], 4 * 4096)):
        assert np.all(np.abs(z.mean(axis=1)) < 0.04) and np.all(np.abs(z.std(axis=1) - 1.0) < 0.04)
        assert abs(np.corrcoef(z[0], z[1])[0, 1]) < 0.04
    # the burst family's sub-tiles: a window is the same stream
    z = ds.brownian_burst_z(11, [5], 3 * 1024)
    assert np.array_equal(ds.brownian_burst_z(11, [5], 1024, 1024), z[:, 1024:2048])
    # the Philox family is philox_normal4 of counter (e // 4, node); per-latent seeds restart the counter in every latent
    zp = ds.brownian_philox_z(11, [9], 12, 2)
    assert np.array_equal(zp[0], ds.philox_normal4(11, 9, np.arange(4)).reshape(-1)[2:14])
    zl = ds.brownian_philox_z(0, [9], 16, 8, latent_seeds=[21, 22], latent_elems=8)
    assert np.array_equal(zl[0, 8:], ds.philox_normal4(22, 9, np.arange(2)).reshape(-1))


# ------------------------------------------------------------------------------------------------ pyramid streams
def _scalar_normal4(words):
    ra, rb, rc, rd = (int(v) for v in words)
    a, b = ds.box_muller(ra, rb)
    c, d = ds.box_muller(rc, rd)
    return [float(a), float(b), float(c), float(d)]


@pytest.mark.parametrize("h, w", [(1, 1), (3, 3), (5, 7), (21, 20), (33, 33)])
def test_pyramid_level_grid_by_a_scalar_walk(h, w):
    """Element i of a drawn level grid, one at a time: slot (i // 4) % 256 of the level's bursts, stepped to round i // 1024, value i % 4 of
    that round's four words -- the burst of (stream_id + 2 + level index, plane, slot)."""
    seed, stream, level, plane = 2**64 - 1, 2**47 + 1, 3, 2**33 + 7
    grid = ds.pyramid_level_grid(seed, stream, level, plane, h, w).reshape(-1)
    n = h * w
    assert grid.shape == (n,)
    for i in sorted({0, min(n - 1, 1), min(n - 1, 2), n - 1, n // 2, min(n - 1, 1023), min(n - 1, 1024), min(n - 1, 1027)}):
        slot, rnd = (i // 4) % 256, i // 1024
        g = ds.rng_stream(seed, stream + 2 + level, plane, slot)
        words = g.words(4 * (rnd + 1))[4 * rnd:]
        assert grid[i] == _scalar_normal4(words)[i % 4], i


def test_pyramid_level_grid_slots_and_keys():
    seed, stream = 2**32 + 5, 2**32 + 3
    # 1089 elements: 256 slots, slot 0 draws a second group (elements 1024 .. 1027) that continues its burst
    g = ds.pyramid_level_grid(seed, stream, 0, 4, 33, 33).reshape(-1)
    burst = ds.rng_stream(seed, stream + 2, 4, 0).words(8)
    assert list(g[:4]) == _scalar_normal4(burst[:4]) and list(g[1024:1028]) == _scalar_normal4(burst[4:])
    assert list(g[4:8]) == _scalar_normal4(ds.rng_stream(seed, stream + 2, 4, 1).words(4))
    # 35 elements: nine slots, the last group cut after three values
    g35 = ds.pyramid_level_grid(seed, stream, 0, 4, 5, 7).reshape(-1)
    assert list(g35[32:]) == _scalar_normal4(ds.rng_stream(seed, stream + 2, 4, 8).words(4))[:3]
    # the level's index in the caller's list and the global plane both key the burst: every value changes
    base = ds.pyramid_level_grid(seed, stream, 1, 4, 21, 20)
    assert np.all(ds.pyramid_level_grid(seed, stream, 2, 4, 21, 20) != base)
    assert np.all(ds.pyramid_level_grid(seed, stream, 1, 5, 21, 20) != base)
    assert np.array_equal(ds.pyramid_level_grid(seed, stream + 1, 0, 4, 21, 20), base)   # stream_id + 2 + index is all that enters
    assert abs(base.std() - 1.0) < 0.1


def test_level_normal_is_a_slot_of_philox_normal4():
    seed, stream = 2**64 - 1, 2**32 + 3
    e = np.array([0, 1, 2, 3, 4, 35, 38, 2**34 + 1, 2**34 + 6])
    z = ds.level_normal(seed, stream, e)
    for i, ei in enumerate(e):
        assert z[i] == ds.philox_normal4(seed, stream, int(ei) // 4)[int(ei) % 4]
    assert ds.level_normal(seed, stream, 7).shape == () and ds.level_normal(seed, stream, e.reshape(3, 3)).shape == (3, 3)
    assert np.all(ds.level_normal(seed, stream + 1, e) != z)


def test_pyramid_planes_of_a_shard_is_the_slice_of_the_whole():
    from tests import pyramid_refs as R

    seed, stream, H, W = 2**32 + 5, 2**47 + 1, 8, 12
    rng = np.random.default_rng(5)
    sup = rng.standard_normal((6, 3, 3))
    levels = [(None, 9, 9, 0.7), (None, H, W, 1.0), (sup, 3, 3, 0.49), (None, 5, 7, -0.3)]
    whole, mag = ds.pyramid_planes(seed, stream, 6, H, W, levels, "bilinear", 0, R.resize, magnitude=True)
    assert whole.shape == mag.shape == (6, H, W) and np.all(mag >= np.abs(whole) - 1e-12)
    for k, n in ((1, 2), (4, 2), (0, 6)):
        shard_levels = [(g if g is None else g[k:k + n], h, w, wt) for g, h, w, wt in levels]
        assert np.array_equal(ds.pyramid_planes(seed, stream, n, H, W, shard_levels, "bilinear", k * H * W, R.resize), whole[k:k + n])
    # the parts: base draw times sqrt(1 + w0^2) in fp32, drawn levels by their index in the caller's list (0 and 3), the supplied one as given
    z = ds.normal_fill(seed, stream, 6 * H * W).reshape(6, H, W) * float(np.sqrt(np.float32(2.0)))
    assert ds.pyramid_base_scale(levels, H, W) == float(np.sqrt(np.float32(2.0))) and ds.pyramid_base_scale(levels[:1], H, W) == 1.0
    g0 = np.stack([ds.pyramid_level_grid(seed, stream, 0, p, 9, 9) for p in range(6)])
    g3 = np.stack([ds.pyramid_level_grid(seed, stream, 3, p, 5, 7) for p in range(6)])
    want = z + float(np.float32(0.7)) * R.resize(g0, H, W, "bilinear") + float(np.float32(0.49)) * R.resize(sup, H, W, "bilinear") \
        + float(np.float32(-0.3)) * R.resize(g3, H, W, "bilinear")
    assert np.allclose(whole, want, rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ Perlin
@pytest.mark.parametrize("blend_mode", ds.PERLIN_BLENDS)
def test_perlin_lattice_is_the_reference_term_of_its_own_angles(blend_mode):
    """perlin_lattice against oracle.sonar_oracle.perlin_term (the reference's cell-centre evaluation, torch fp64) of the angles
    perlin_lattice_revolutions states, summed over the iterations; the draws by a scalar walk of the counter rule."""
    import torch

    from oracle import sonar_oracle as orc

    seed, stream, iters, C, H, W = 2**32 + 5, 2**47 + 1, 6, 2, 5, 7
    rev = ds.perlin_lattice_revolutions(seed, stream, iters, C, H, W)
    assert rev.shape == (iters, C, H + 1, W + 1) and rev.min() >= 0.0 and rev.max() < 1.0
    for it, c, gy, gx in ((0, 0, 0, 0), (3, 1, 5, 7), (4, 0, 2, 3), (5, 1, 0, 6)):
        p = (c * (H + 1) + gy) * (W + 1) + gx
        w = ds.philox4x32_10(p, 0, it // 4, stream & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)
        assert rev[it, c, gy, gx] == ds.u01(w[it % 4])
    want = sum(orc.perlin_term(torch.from_numpy(2.0 * math.pi * rev[it]), blend_mode) for it in range(iters)).numpy()
    got = ds.perlin_lattice(seed, stream, iters, C, H, W, blend_mode)
    assert got.shape == (C, H, W) and np.max(np.abs(got - want)) < 1e-14
    assert np.array_equal(ds.perlin_lattice(seed, stream, 0, C, H, W, blend_mode), np.zeros((C, H, W)))
    # a prefix of the iterations is a prefix of the sum: iteration `it` does not depend on how many follow
    assert np.allclose(ds.perlin_lattice(seed, stream, 5, C, H, W, blend_mode) + ds.perlin_cell_terms(rev[5], blend_mode), got, rtol=0, atol=1e-14)


def test_perlin_lattice_takes_the_low_word_of_the_stream_id():
    a = ds.perlin_lattice_revolutions(7, 3, 5, 1, 3, 4)
    assert np.array_equal(a, ds.perlin_lattice_revolutions(7, 2**32 + 3, 5, 1, 3, 4))
    assert np.all(a != ds.perlin_lattice_revolutions(7, 4, 5, 1, 3, 4)) and np.all(a != ds.perlin_lattice_revolutions(2**32 + 7, 3, 5, 1, 3, 4))


def test_perlin_values_windows_are_slices_of_the_whole_call():
    seed, stream, chw, B, off = 2**64 - 1, 2**32 + 3, 260, 40, 3 * 260
    n = B * chw
    terms = np.random.default_rng(2).standard_normal((2, chw)).astype(np.float32)
    whole, steps = ds.perlin_values(seed, stream, terms, chw, 1.5, n, off)
    u = ds.uniform_fill(seed, stream, n, off).astype(np.float64)
    pos = np.arange(n) % chw
    assert np.array_equal(whole, u / float(np.float32(1.5)) + terms[0].astype(np.float64)[pos] + terms[1].astype(np.float64)[pos])
    for first, count in ((0, 1), (4095, 2), (4096 - off, 4096), (n - 5, 5), (777, 3000)):
        part, psteps = ds.perlin_values(seed, stream, terms, chw, 1.5, n, off, first, count)
        assert np.array_equal(part, whole[first:first + count]) and np.array_equal(psteps(), steps()[first:first + count])
    # a shard is the slice of the batch: the tables repeat per latent, the words follow the global element
    shard, _ = ds.perlin_values(seed, stream, terms, chw, 1.5, 10 * chw, off + 7 * chw)
    assert np.array_equal(shard, whole[7 * chw:17 * chw])
    # one table given flat, and none at all
    one, _ = ds.perlin_values(seed, stream, terms[0], chw, 2.0, n, off)
    assert np.array_equal(one, u / 2.0 + terms[0].astype(np.float64)[pos])
    none, nsteps = ds.perlin_values(seed, stream, np.zeros((0, chw), np.float32), chw, -4.0, n, off)
    assert np.array_equal(none, u / -4.0) and np.array_equal(nsteps().astype(np.float64), none)


@pytest.mark.parametrize("div_fac", [2.0, 0.5, 1.0, -4.0, 1.5, 3.0, -1.7])
def test_perlin_float32_steps_stay_within_the_rounding_bound(div_fac):
    seed, stream, chw, n = 5, 2**47 + 1, 1024, 3 * 1024
    rng = np.random.default_rng(11)
    assert ds.divisor_is_power_of_two(div_fac) == (div_fac in (2.0, 0.5, 1.0, -4.0))
    for terms in (rng.standard_normal((1, chw)).astype(np.float32), rng.standard_normal((3, chw)).astype(np.float32), np.zeros((0, chw), np.float32)):
        value, steps = ds.perlin_values(seed, stream, terms, chw, div_fac, n, 64)
        bound = ds.perlin_rounding_bound(seed, stream, terms, chw, div_fac, n, 64)
        got = steps()
        assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - value) <= bound)
        assert np.max(np.abs(got.astype(np.float64) - value)) < 2e-6  # (the bound is a few ulps of values of size ~3, not a loose one)
        if terms.shape[0] == 1:
            assert np.array_equal(steps(fused=True), got)  # a power of two: one rounding of the exact sum is the rounded steps' bits


# ------------------------------------------------------------------------------------------------ half-spectrum draw orders
@pytest.mark.parametrize("shape", list(ds.FIXED_PLANES) + [(104, 152), (96, 168), (256, 256)])
def test_every_half_spectrum_element_is_drawn_once(shape):
    H, W = shape
    kind = 1 if shape in ds.FIXED_PLANES else 4 if shape == (256, 256) else 2
    counts, discarded = ds.spectrum_draw_order(H, W, kind)
    assert counts.shape == (H, W // 2 + 1) and counts.min() == 1 and counts.max() == 1
    assert discarded == (H // 2 if kind in (1, 2) else 0)  # only the kx = M pair slot of each row pair
    if kind == 1:
        assert H <= ds.plane_threads(H, W)  # edge rows are slots of the workgroup


def test_spectrum_draws_are_unit_complex_normals_keyed_by_group():
    z = ds.spectrum_draws(3, 2**32 + 3, 8, 64, 64, 0, 4, 1)
    assert np.all(z != 0) and abs(np.mean(np.abs(z) ** 2) - 1.0) < 0.02
    # a plane's values depend on its global index only: a window of planes at an offset matches
    assert np.array_equal(ds.spectrum_draws(3, 2**32 + 3, 3, 64, 64, 5, 4, 1), z[5:8])
    assert np.array_equal(ds.spectrum_draws(3, 7, 2, 104, 152, 1, 1, 2), ds.spectrum_draws(3, 7, 3, 104, 152, 0, 1, 2)[1:])


# ------------------------------------------------------------------------------------------------ host expansion vs the oracle tree
def _grid_queries(rnd, lo, hi, D, k):
    cells = 1 << D
    ts = [lo + rnd.randrange(1, cells) * (hi - lo) / cells for _ in range(k)]
    ts += [rnd.uniform(lo, hi) for _ in range(k)]
    ts += [lo, hi, hi + 0.3 * (hi - lo) / cells, lo - 0.3 * (hi - lo) / cells]  # ends, and times that snap onto them
    ts += ts[:5]                                                                   # repeated queries
    rnd.shuffle(ts)
    return ts


@pytest.mark.parametrize("D", [24, 6])
def test_brownian_path_equals_the_oracle_tree(pkg, D):
    import importlib

    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    lo, hi = 0.0292, 14.6146
    rnd = random.Random(D)
    bp = ng.BrownianPath(lo, hi, D)
    assert bp.tree_depth == D

    def close(got, want):
        keys = set(got) | set(want)
        assert all(abs(got.get(k, 0.0) - want.get(k, 0.0)) <= 1e-12 for k in keys), (got, want)

    ts = _grid_queries(rnd, lo, hi, D, 40)
    for t in ts:
        close(bp.coefficients(t), ds.tree_point(lo, hi, D, bp.grid_index(bp.resolve(t))))
    for t0, t1 in zip(ts[:-1], ts[1:]):
        g0, g1 = bp.grid_index(bp.resolve(t0)), bp.grid_index(bp.resolve(t1))
        if g0 == g1:
            continue
        ids, co = bp.increment(t0, t1)
        want = {k: v for k, v in ds.tree_increment(lo, hi, D, g0, g1).items() if abs(v) > 1e-12}
        close(dict(zip(ids, co)), want)
    # the oracle tree is a Brownian motion: Var W(t) = t - t_lo
    for g in (1, 5, (1 << D) - 1):
        c = ds.tree_point(lo, hi, D, g)
        assert math.isclose(sum(v * v for v in c.values()), ds.tree_grid_time(lo, hi, D, g) - lo, rel_tol=1e-12)
