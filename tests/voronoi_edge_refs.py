"""What tests/test_voronoi_edges_cpu.py and tests/test_gpu_voronoi_edges.py share beyond the case table (tests only, numpy): the inputs of
a case, its fp64 and fp32 statements (tests/voronoi_refs.py, tests/voronoi_rank_refs.py: computed once, shared and left unchanged), the
accumulation every launch performs, and the deliberately wrong statements of the negative controls.

``Probe`` is the statement's Octave with its intermediate tensors kept: the fuzz term's inner distance, the fuzzed distance before the
rescale (what fuzz passes 0 and 1 reduce) and the distance the result program reads.  Its ``_fuzzed`` is the base class's, step for step,
with one switch: ``keep`` [H, W] restricts the per-row extremes to some pixels (negative control: a workgroup's share of a row lost)."""
from __future__ import annotations

import collections

import numpy as np

from oracle import device_streams as ds
from tests import voronoi_edge_cases as E
from tests import voronoi_rank_refs as RR
from tests import voronoi_refs as R

NEAR_OFFSET = np.array([0.003, 0.002, 0.001])
FAR_OFFSET = np.array([0.499, 0.499, 0.499])


def points(tag, n, rank):
    """The feature points [B, C, n, 3] of a case, fp32; E.PLACE says where the last one goes."""
    B, C, H, W = E.SHAPES[tag]
    fp = np.random.default_rng(E.SEED_RANK if rank else E.SEED_TOP).random((B, C, n, 3), dtype=np.float32)
    place = E.PLACE.get((tag, bool(rank)))
    if place is not None:
        kind, y, x = place
        at = np.array([y / H, x / W, E.Z_NORM]) + (NEAR_OFFSET if kind == "near" else FAR_OFFSET)
        fp[:, :, -1, :] = (at % 1.0).astype(np.float32)
    return fp


def base(tag):
    """What the launch accumulates into: random, non-zero."""
    return np.random.default_rng(E.SEED_BASE).random(E.SHAPES[tag], dtype=np.float32) + np.float32(0.5)


def uniforms(tag, n):
    """Replay mode's drawn uniforms [B, C, H, W, n]."""
    return np.random.default_rng(E.SEED_U).random((*E.SHAPES[tag], n), dtype=np.float32)


def stream_draw(offset, wrong=None):
    """``draw(shape)`` of the statements: the uniforms sonar_philox_uniform_f32 fills for the case's stream from ``offset`` on.  ``wrong``:
    "offset0" reads them from element 0, "mod_tile" takes the element index modulo the stream's tile (negative controls)."""

    def draw(shape):
        n = int(np.prod(shape))
        if wrong == "mod_tile":
            tile = ds.uniform_fill(E.STREAM_SEED, E.STREAM_ID, ds.TILE_ELEMS, 0)
            return tile[(offset + np.arange(n, dtype=np.int64)) % ds.TILE_ELEMS].reshape(shape)
        return ds.uniform_fill(E.STREAM_SEED, E.STREAM_ID, n, 0 if wrong == "offset0" else offset).reshape(shape)

    return draw


def _probe(parent):
    class Probe(parent):
        keep = None
        inner = fuzzed = dist = None

        def _fuzzed(self, result, fuzz):
            T = self.T
            self.inner = result.copy()
            rmin, rmax = float(result.min()), float(result.max())
            fz = max(abs(rmin), abs(rmax)) * float(fuzz)
            result += self.draw(result.shape).astype(T) * self.c(fz * 2) - self.c(fz)
            self.fuzzed = result.copy()
            if self.keep is None:
                lo, hi = result.min(axis=(-2, -1), keepdims=True), result.max(axis=(-2, -1), keepdims=True)
            else:
                keep = self.keep[None, None, :, :, None]
                lo = np.where(keep, result, np.inf).min(axis=(-2, -1), keepdims=True).astype(T)
                hi = np.where(keep, result, -np.inf).max(axis=(-2, -1), keepdims=True).astype(T)
            out = (result - lo) / ((hi - lo) + self.c(1e-07))
            out = out * T(np.float32(rmax - rmin)) + self.c(rmin)
            return np.clip(out, self.c(rmin), self.c(rmax))

        def result(self, d, d_orig, expr):
            self.dist = d.copy()
            return super().result(d, d_orig, expr)

    return Probe


PROBES = {False: _probe(R.Octave), True: _probe(RR.Octave)}
Statement = collections.namedtuple("Statement", "want amb got32 err32 bound o64 o32")


def accumulate(val, into, T):
    """The launch's epilogue: (base + result * amplitude) / final_div."""
    return (into.astype(T) + val * T(np.float32(E.AMPLITUDE))) / T(np.float32(E.FINAL_DIV))


def statement(rank, tag, fp, dmode, rmode, scale, *, draw=None, keep=None, into=None):
    """The fp64 statement of one launch, its flags, the fp32 statement, the yardstick and R.bound of it.  ``into``: the launch accumulates
    (``accumulate``) instead of writing into zeros with amplitude 1."""
    _b, _c, H, W = E.SHAPES[tag]
    runs = []
    for T in (np.float64, np.float32):
        o = PROBES[rank](T, None, draw)
        o.keep = keep
        out, amb = o.run(fp, H, W, E.Z_NORM, scale, dmode, rmode)
        runs.append((o, out if into is None else accumulate(out, into, T), amb))
    (o64, want, amb), (o32, got32, _) = runs
    assert want.dtype == np.float64 and got32.dtype == np.float32
    err32 = R.error(got32, want, amb)
    return Statement(want, amb, got32, err32, R.bound(err32, want), o64, o32)


_cache = {}


def case_statement(rank, case):
    """``statement`` of a case of E.OCTAVE / E.RANK with its own points and base: (fp, base, Statement), computed once."""
    key = (rank, case[0])
    if key not in _cache:
        _name, tag, n, dmode, rmode, scale = case
        fp, into = points(tag, n, rank), base(tag)
        _cache[key] = (fp, into, statement(rank, tag, fp, dmode, rmode, scale, into=into))
    return _cache[key]


def replay_statement(case):
    """``statement`` of a case of E.FUZZ_REPLAY on its replay uniforms: (fp, u, Statement), computed once."""
    key = ("replay", case[0])
    if key not in _cache:
        _name, tag, n, dmode, rmode, scale, _exact = case
        fp, u = points(tag, n, False), uniforms(tag, n)
        _cache[key] = (fp, u, statement(False, tag, fp, dmode, rmode, scale, draw=lambda shape: u.reshape(shape)))
    return _cache[key]


def encode(values):
    """fp32 values as the kernel's ordered integers (unsigned, of the floats' order)."""
    b = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def statistics_words(o32):
    """The statistics buffer after fuzz passes 0 and 1 as the fp32 statement has it: [0] / [1] the inner distance's whole-tensor minimum and
    maximum, [2 + 2 r] / [3 + 2 r] the fuzzed distance's of row r = (b, c, y)."""
    assert o32.T is np.float32
    lo, hi = o32.fuzzed.min(axis=(-2, -1)).reshape(-1), o32.fuzzed.max(axis=(-2, -1)).reshape(-1)
    words = np.empty(2 + 2 * lo.size, np.uint32)
    words[:2] = encode([o32.inner.min(), o32.inner.max()])
    words[2::2], words[3::2] = encode(lo), encode(hi)
    return words


def first_tile_only(tag, block):
    """keep [H, W]: of every row the pixels that lie in the same ``block``-pixel tile as the row's first pixel."""
    _b, _c, H, W = E.SHAPES[tag]
    pix = np.arange(H * W).reshape(H, W)
    return pix // block == (pix[:, :1] // block)


def planes_by_unit_modulo(right, swapped, block):
    """What a kernel that took ``plane = unit % planes`` instead of ``unit / tiles`` would write on two planes: ``swapped`` is the statement
    with the two planes' points exchanged."""
    _b, planes, H, W = right.shape
    assert planes == 2 and right.shape[0] == 1
    tiles = -(-H * W // block)
    out = right.reshape(planes, H * W).copy()
    other = swapped.reshape(planes, H * W)
    for unit in range(planes * tiles):
        plane, tile = divmod(unit, tiles)
        if unit % planes != plane:
            out[plane, tile * block:(tile + 1) * block] = other[plane, tile * block:(tile + 1) * block]
    return out.reshape(right.shape)
