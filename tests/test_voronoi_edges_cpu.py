"""CPU: the cases of tests/voronoi_edge_cases.py, before tests/test_gpu_voronoi_edges.py launches them.

  * Geometry: from the kernels' own constants (the 256-thread block, the 2048-workgroup cap and the 64-lane wave of csrc/common.h, the row
    instantiation's 64-pixel tile of csrc/voronoi.hip, hip_lib.VORONOI_*, the stream tile of oracle/device_streams.py) every tag reaches the
    edge it is named for.  If a constant changes, this fails instead of the GPU tests quietly losing their coverage.
  * The statements' flagged share stays under the cases' caps (1e-3; 1e-2 for cellid and the angle distance), so the bound of
    tests/voronoi_refs.py judges (nearly) every element; the fp32 yardstick and the bound of every case are printed.
  * Negative controls: a statement with one deliberate geometry error -- a row's extremes from one workgroup's pixels only, uniforms read
    from element 0 or modulo the stream tile, the last feature point dropped, the plane taken as unit % planes -- lands outside R.bound of the
    right one (or differs in the statistics words): the shapes tell a wrong kernel from a right one."""
import os
import re

import numpy as np
import pytest

from oracle import device_streams as ds
from tests import voronoi_edge_cases as E
from tests import voronoi_edge_refs as X
from tests import voronoi_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "comfyui-sonar_amd", "csrc")


def constant(header, name):
    """``constexpr int name = a * b ...;`` of a kernel source: the product."""
    text = re.sub(r"//.*", "", open(os.path.join(CSRC, header)).read())
    found = re.search(rf"constexpr int {name} = ([0-9 *]+);", text)
    assert found is not None, f"{name} is not a constant of {header}"
    return int(np.prod([int(v) for v in found.group(1).split("*")]))


@pytest.fixture(scope="module")
def K(pkg):
    hl = pkg.hip_lib
    k = dict(block=constant("common.h", "kBlock"), wave=constant("common.h", "kWave"), max_grid=constant("common.h", "kMaxGrid"),
             row_lanes=constant("voronoi.hip", "kRowLanes"), chunk=hl.VORONOI_CHUNK, max_points=hl.VORONOI_MAX_POINTS,
             row_n=hl.VORONOI_RANK_ROW_N, tile_elems=ds.TILE_ELEMS)
    text = open(os.path.join(CSRC, "voronoi.hip")).read()
    assert "constexpr int kChunk = SONAR_VORONOI_CHUNK;" in text and "static_assert(kChunk == kBlock" in text
    assert constant("common.h", "kTileIters") * 256 == k["tile_elems"]
    return k


def waves(hw, W, K):
    """Per live wave of the 256-pixel tiles: the rows its live pixels lie in."""
    for first in range(0, hw, K["wave"]):   # (a tile is a whole number of waves)
        pix = np.arange(first, min(first + K["wave"], hw))
        yield np.unique(pix // W)


def facts(tag, n, K):
    B, C, H, W = E.SHAPES[tag]
    hw, planes = H * W, B * C
    tiles, row_tiles = -(-hw // K["block"]), -(-hw // K["row_lanes"])
    rows_of_waves = list(waves(hw, W, K))
    tile_of = np.arange(hw).reshape(H, W) // K["block"]
    extent = B * C * hw * n
    assert K["block"] % K["wave"] == 0
    return {
        "tiles": tiles > 1,
        "ragged_tile": tiles > 1 and hw % K["block"] != 0,
        "row_tiles_ragged": row_tiles > 2 and hw % K["row_lanes"] != 0,
        "waves_straddle_rows": 2 * sum(len(rows) > 1 for rows in rows_of_waves) > len(rows_of_waves),   # most of them
        "waves_inside_rows": all(len(rows) == 1 for rows in rows_of_waves),
        "row_in_two_tiles": bool((tile_of.min(axis=1) != tile_of.max(axis=1)).any()),
        "row_is_a_wave": W == K["wave"] and all(len(rows) == 1 for rows in rows_of_waves),
        "second_unit": planes * tiles > K["max_grid"],
        "row_second_unit": planes * row_tiles > K["max_grid"],
        "full_chunks": n == K["max_points"] and n % K["chunk"] == 0 and n // K["chunk"] == 16,
        "chunks": n > K["chunk"] and n % K["chunk"] == 1,
        "stream_tile": extent > K["tile_elems"],
        "stream_two_boundaries": extent > 2 * K["tile_elems"],
        # a second trip of the plane kernels' grid-stride loops, whose stride is more than one row and no whole number of rows or planes
        "plane_second_trip": (planes * hw > K["max_grid"] * K["block"] > W and (K["max_grid"] * K["block"]) % W != 0
                              and (K["max_grid"] * K["block"]) % hw != 0),
    }


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("tag, n, reaches", E.REACHES, ids=[f"{t}_n{n}" for t, n, _r in E.REACHES])
def test_every_tag_reaches_the_edges_it_is_named_for(K, tag, n, reaches):
    have = facts(tag, n, K)
    for fact in reaches:
        assert have[fact], f"{tag} with {n} points no longer reaches {fact}: {K}"


def test_the_case_table_uses_the_tags_as_stated(K):
    used = {(c[1], c[2]) for table in (E.OCTAVE, E.FUZZ_REPLAY, E.STREAM, E.RANK_STREAM, E.RANK) for c in table}
    used |= {(t, n) for t, n, _d, _r in E.TOP_FOUR}
    stated = {(t, n) for t, n, _r in E.REACHES}
    assert {(t, n) for t, n in used if n in (2, 4096) or t in ("R192", "R64", "N257F")} <= stated
    assert {t for t, _n in used} == set(E.SHAPES) - {"P"}
    ids = [c[0] for table in (E.OCTAVE, E.FUZZ_REPLAY, E.RANK) for c in table]
    assert len(ids) == len(set(ids)) and E.WIDE <= set(ids) | {c[0] for c in E.STREAM}
    # the row instantiation takes a whole plane's points from one staged chunk
    assert all(n <= K["row_n"] for _i, _t, n, _d, r, *_ in (*E.RANK, *E.RANK_STREAM) if "use_sorted" in r)
    # a shard's element offsets: inside a group of four, at a stream tile's last group, past 2^33
    assert {o % 4 for o in E.OFFSETS} >= {0, 1, 3} and any(o % K["tile_elems"] >= K["tile_elems"] - 4 for o in E.OFFSETS)
    assert max(E.OFFSETS) > 2**33 and E.STREAM_ID > 2**32 and E.STREAM_SEED > 2**32
    # generate mode under shard_offset(1): the fuzz draw of the generator cases starts past a stream tile, inside a group of four
    for _name, _rank, latent, params in E.GENERATOR:
        per_latent = int(np.prod(latent[1:])) * params["n_points"][0]
        assert per_latent > K["tile_elems"] and per_latent % 4 != 0


# ------------------------------------------------------------------------------------------------ the flagged share and the yardstick
def report(name, st):
    share = float(st.amb.mean())
    print(f"{name}: fp32 statement {st.err32:.3e}  bound {st.bound:.3e}  ambiguous {share:.2e}")
    return share


def cap(name):
    return E.CAP_WIDE if name in E.WIDE else E.CAP


@pytest.mark.parametrize("case", E.OCTAVE, ids=[c[0] for c in E.OCTAVE])
def test_flagged_share_of_the_octave_cases(case):
    _fp, _into, st = X.case_statement(False, case)
    assert report(case[0], st) <= cap(case[0]) and np.isfinite(st.want).all() and st.err32 > 0.0


@pytest.mark.parametrize("case", E.RANK, ids=[c[0] for c in E.RANK])
def test_flagged_share_of_the_rank_cases(case):
    _fp, _into, st = X.case_statement(True, case)
    assert report(case[0], st) <= cap(case[0]) and np.isfinite(st.want).all() and st.err32 > 0.0


@pytest.mark.parametrize("case", E.FUZZ_REPLAY, ids=[c[0] for c in E.FUZZ_REPLAY])
def test_flagged_share_of_the_replayed_fuzz_cases(case):
    _fp, _u, st = X.replay_statement(case)
    assert report(case[0], st) <= cap(case[0]) and np.isfinite(st.want).all() and st.err32 > 0.0


def stream_statement(rank, case, offset, wrong=None, fp=None, draw=None):
    _name, tag, n, dmode, rmode = case
    fp = X.points(tag, n, rank) if fp is None else fp
    return X.statement(rank, tag, fp, dmode, rmode, 1.0, draw=X.stream_draw(offset, wrong) if draw is None else draw)


_right = {}


def right(rank, case, offset):
    key = (rank, case[0], offset)
    if key not in _right:
        _right[key] = stream_statement(rank, case, offset)
    return _right[key]


@pytest.mark.parametrize("rank, case", [(False, c) for c in E.STREAM] + [(True, c) for c in E.RANK_STREAM],
                         ids=[c[0] for c in E.STREAM] + ["rank_" + c[0] for c in E.RANK_STREAM])
def test_flagged_share_of_the_stream_cases(rank, case):
    for offset in E.OFFSETS:
        st = right(rank, case, offset)
        assert report(f"{case[0]} offset {offset}", st) <= cap(case[0]) and np.isfinite(st.want).all()


def test_the_probe_is_the_statement():
    """The Octave of tests/voronoi_edge_refs.py restates _fuzzed to keep its intermediate tensors: the same bits as the base class."""
    _name, tag, n, dmode, rmode = E.STREAM[1]
    _b, _c, H, W = E.SHAPES[tag]
    fp = X.points(tag, n, False)
    st = right(False, E.STREAM[1], 175)
    for T, mine in ((np.float64, st.want), (np.float32, st.got32)):
        out, _amb = R.Octave(T, None, X.stream_draw(175)).run(fp, H, W, E.Z_NORM, 1.0, dmode, rmode)
        assert np.array_equal(out, mine)
    assert np.array_equal(X.encode(np.float32([-1.5, -0.0, 0.0, 2.0])), np.uint32([0x403FFFFF, 0x7FFFFFFF, 0x80000000, 0xC0000000]))


# ------------------------------------------------------------------------------------------------ negative controls
def outside(wrong32, st, amb=None):
    """A kernel that computed ``wrong32`` would fail the GPU test's assertion against the right statement."""
    err = R.error(wrong32, st.want, st.amb if amb is None else st.amb | amb)
    return err > st.bound, err


def test_a_row_that_loses_one_workgroups_share_is_noticed(K):
    """(a) R192: row 1 lies in tiles 0 and 1.  Extremes taken from the first tile's pixels alone change the row's statistics words and push
    pass 2 out of bound."""
    for case in (c for c in E.FUZZ_REPLAY if c[1] == "R192"):
        _name, tag, n, dmode, rmode, scale, _exact = case
        fp, u, st = X.replay_statement(case)
        keep = X.first_tile_only(tag, K["block"])
        assert not keep.all() and keep[0].all() and keep[:, 0].all()
        wrong = X.statement(False, tag, fp, dmode, rmode, scale, draw=lambda shape: u.reshape(shape), keep=keep)
        words, bad = X.statistics_words(st.o32), np.where(keep[None, None, :, :, None], wrong.o32.fuzzed, np.nan)
        lo, hi = np.nanmin(bad, axis=(-2, -1)).reshape(-1), np.nanmax(bad, axis=(-2, -1)).reshape(-1)
        rows = (X.encode(lo) != words[2::2]) | (X.encode(hi) != words[3::2])
        far, err = outside(wrong.got32, st)
        print(f"{case[0]}: rows with other statistics {rows.sum()} of {rows.size}, pass 2 at {err:.3e} for a bound of {st.bound:.3e}")
        assert rows.any() and not rows.reshape(-1, keep.shape[0])[:, 0].any() and far


@pytest.mark.parametrize("rank, case", [(False, c) for c in E.STREAM] + [(True, c) for c in E.RANK_STREAM],
                         ids=[c[0] for c in E.STREAM] + ["rank_" + c[0] for c in E.RANK_STREAM])
def test_uniforms_from_the_wrong_stream_element_are_noticed(rank, case):
    """(b) the element offset ignored, (c) the element index taken modulo the stream tile: both out of bound at every offset they change."""
    for offset in E.OFFSETS:
        st = right(rank, case, offset)
        for wrong in ("offset0", "mod_tile"):
            if wrong == "offset0" and offset == 0:
                continue
            bad = stream_statement(rank, case, offset, wrong)
            far, err = outside(bad.got32, st, bad.amb)
            print(f"{case[0]} offset {offset} {wrong}: {err:.3e} for a bound of {st.bound:.3e}")
            assert far, (offset, wrong)


def last_point_rank(o64):
    """Per pixel, how many points lie nearer than the last one (by the distance the result program reads)."""
    return (o64.dist[..., :-1] < o64.dist[..., -1:]).sum(axis=-1)


DROPS = [(False, c) for c in E.OCTAVE if c[1] == "N4096"] + [(True, c) for c in E.RANK if c[1] == "N4096"]


@pytest.mark.parametrize("rank, case", DROPS, ids=[("rank_" if r else "") + c[0] for r, c in DROPS])
def test_a_dropped_last_point_is_noticed_at_4096_points(rank, case):
    """(d) the last point of the sixteenth chunk is the nearest of pixel (2, 3) (the farthest where the case reads the last rank)."""
    _name, tag, n, dmode, rmode, scale = case
    fp, into, st = X.case_statement(rank, case)
    place = E.PLACE[(tag, rank)]
    ranks = last_point_rank(st.o64)
    assert ranks.shape == E.SHAPES[tag] and not st.amb[0, 0, place[1], place[2]]
    assert ranks[0, 0, place[1], place[2]] == (0 if place[0] == "near" else n - 1)
    assert bool(((ranks < 4) & ~st.amb).any()) or place[0] == "far"
    bad = X.statement(rank, tag, fp[:, :, :-1], dmode, rmode, scale, into=into)
    far, err = outside(bad.got32, st, bad.amb)
    print(f"{case[0]}: without the last point {err:.3e} for a bound of {st.bound:.3e}")
    assert far


@pytest.mark.parametrize("rank, case", [(r, c) for r, t in ((False, E.STREAM), (True, E.RANK_STREAM)) for c in t if c[1] == "N257F"],
                         ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_a_dropped_last_point_is_noticed_at_257_points(rank, case):
    """(d) the single point of the second chunk, with the uniforms of the points that stay left where they are."""
    _name, tag, n, _dmode, _rmode = case
    offset = E.OFFSETS[1]
    st = right(rank, case, offset)
    ranks = last_point_rank(st.o64)
    print(f"{case[0]}: the last point is among the four nearest of {int(((ranks < 4) & ~st.amb).sum())} pixels")
    assert bool(((ranks < 4) & ~st.amb).any())
    full = X.stream_draw(offset)
    bad = stream_statement(rank, case, offset, fp=X.points(tag, n, rank)[:, :, :-1],
                           draw=lambda shape: full((*shape[:-1], shape[-1] + 1))[..., :-1])
    far, err = outside(bad.got32, st, bad.amb)
    print(f"{case[0]}: without the last point {err:.3e} for a bound of {st.bound:.3e}")
    assert far


def test_a_plane_taken_as_unit_modulo_planes_is_noticed(K):
    """(e) T3: 2 planes of 3 tiles.  unit % planes instead of unit / tiles reads the other plane's points in three of the six units."""
    for rank, case in ((False, E.OCTAVE[0]), (False, E.OCTAVE[2]), (True, E.RANK[0])):
        _name, tag, n, dmode, rmode, scale = case
        assert tag == "T3"
        fp, into, st = X.case_statement(rank, case)
        swapped = X.statement(rank, tag, np.ascontiguousarray(fp[:, ::-1]), dmode, rmode, scale, into=into)
        bad = X.planes_by_unit_modulo(st.got32, swapped.got32, K["block"])
        changed = (bad != st.got32).reshape(2, -1).any(axis=1)
        far, err = outside(bad, st, swapped.amb)
        print(f"{case[0]}: {err:.3e} for a bound of {st.bound:.3e}")
        assert changed.all() and far and not outside(st.got32, st)[0]
