"""-m gpu: the two-point Brownian query -- ``BrownianTreeNoiseSampler.pair`` / ``sonar_brownian_pair_f32`` / SonarDPMPPSDE's prefetch.

``pair`` is observationally two calls: the launcher merges the two points' expansions by node id, the kernel draws each node once and
accumulates every point in ascending id order from its own base -- the single-point kernel's operation sequence.  No sum is reassociated, so
every comparison here is ``torch.equal`` (the tolerance the issue allows for a reassociated shared sum is not needed)."""
import importlib
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
LO, HI = 0.03, 14.6
SCHEDULE = [HI, 9.1, 5.2, 2.3, 0.9, 0.2, LO]  # 6 steps: no kept point at the first, a kept W(sigma) afterwards, t_lo at the last


@pytest.fixture(scope="module")
def api(pkg):
    pkg.hip_lib.load()
    mods = {m: importlib.import_module(f"comfyui_sonar_amd.py.{m}") for m in ("utils", "noise_generation", "noise", "sonar")}
    return types.SimpleNamespace(**mods, hl=pkg.hip_lib)


def mid(s, s_next):
    """DPM++ SDE's half-step sigma (r = 1/2 in log sigma)."""
    return math.sqrt(s * s_next)


def counted(monkeypatch, hl):
    """Launch counts by entry point, increments only (``want_out``: the kept-tensor evaluations of the coarse grid write no increment)."""
    calls = {"pair": 0, "single": 0}
    real = {k: getattr(hl, k) for k in ("brownian_pair", "brownian_point", "brownian_bridge")}

    def wrap(name, key):
        def fn(*a, **k):
            if key == "pair" or k.get("want_out", True):
                calls[key] += 1
            return real[name](*a, **k)
        monkeypatch.setattr(hl, name, fn)

    wrap("brownian_pair", "pair")
    wrap("brownian_point", "single")
    wrap("brownian_bridge", "single")
    return calls


@pytest.mark.parametrize("stats", [False, True], ids=["plain-draw", "with-statistics"])
@pytest.mark.parametrize("shape,seed", [((2, 4, 32, 32), 11), ((1, 4, 16, 16), 12), ((3, 3, 10, 14), 13), ((2, 4, 32, 32), [5, 6])],
                         ids=["burst-2-tiles", "burst-1-tile", "plain", "per-latent-seeds"])
def test_pair_equals_two_calls_over_a_schedule(api, monkeypatch, shape, seed, stats):
    """Statistics are reduced per block, so their slots are the two calls' bits only when each increment is written by a launch of the shape
    its own call would make: with them, the first step (W(sigma) not kept yet: the first call's increment comes from the launch that
    evaluates W(sigma)) and the last (W(t_lo) has no terms, the half step's point has twenty: two block sizes) keep their two calls."""
    ng = api.noise_generation
    x = torch.zeros(shape, device="cuda")
    one, two = (ng.BrownianTreeNoiseSampler(x, LO, HI, seed=seed, tree_depth=24) for _ in range(2))
    calls = counted(monkeypatch, api.hl)
    for s, s_next in zip(SCHEDULE, SCHEDULE[1:]):
        before = dict(calls)
        parts, parts2 = (tuple(api.hl.new_partials("cuda") for _ in range(2)) if stats else None for _ in range(2))
        a, b = one.pair(s, mid(s, s_next), s_next, partials=parts)
        if stats and (s == HI or s_next == LO):
            assert calls["pair"] == before["pair"] and calls["single"] == before["single"] + 2
        else:
            assert calls["pair"] == before["pair"] + 1 and calls["single"] == before["single"], "one launch makes both increments"
        a2, b2 = two(s, mid(s, s_next), partials=parts2 and parts2[0]), two(s, s_next, partials=parts2 and parts2[1])
        assert torch.equal(a, a2) and torch.equal(b, b2), (s, s_next)
        assert not stats or all(torch.equal(p, q) for p, q in zip(parts, parts2)), "the statistics slots too"
        assert a.data_ptr() != b.data_ptr() and abs(a.std().item() - 1) < 0.2 and abs(b.std().item() - 1) < 0.2
        assert list(one._points) == list(two._points) and all(torch.equal(one._points[t], two._points[t]) for t in one._points)
    assert one.path.t_lo in one._points  # (the last step evaluated and kept W(t_lo) = 0, as the two calls do)


def test_four_byte_aligned_buffers_take_the_same_values(api):
    """Views at an odd storage offset for prev and the bases: the burst family with 4-byte accesses, the same bits as the aligned call and as
    two single-point calls on the same views."""
    hl = api.hl
    shape, n = (2, 4, 32, 32), 2 * 4 * 32 * 32
    g = torch.Generator(device="cuda").manual_seed(3)
    odd = lambda: torch.randn(n + 1, device="cuda", generator=g)[1:].view(shape)  # noqa: E731
    prev, wa, wb = odd(), odd(), odd()
    assert prev.data_ptr() % 16 == 4
    lists = dict(shared=([40], [0.3]), only_1=([17, 35, 70, 141], [0.5, -0.25, 0.125, 0.7]), only_2=([17, 34, 69], [0.4, 0.2, -0.6]))
    kw = dict(base_1=(wa, 0.25, wb, 0.75), base_2=(wa, 0.5, None, 0.0), prev=prev, scale_1=1.5, scale_2=-0.5)
    (a, w1), (b, w2) = hl.brownian_pair(shape, "cuda", lists["shared"], lists["only_1"], lists["only_2"], 77, 0, None, **kw)
    al = {k: v.clone() for k, v in dict(prev=prev, wa=wa, wb=wb).items()}
    (a_al, _), (b_al, _) = hl.brownian_pair(shape, "cuda", lists["shared"], lists["only_1"], lists["only_2"], 77, 0, None,
                                            base_1=(al["wa"], 0.25, al["wb"], 0.75), base_2=(al["wa"], 0.5, None, 0.0), prev=al["prev"], scale_1=1.5,
                                            scale_2=-0.5)
    assert torch.equal(a, a_al) and torch.equal(b, b_al)
    merged = lambda only: sorted(zip(lists["shared"][0] + only[0], lists["shared"][1] + only[1]))  # noqa: E731
    for (out, w), only, base, scale in (((a, w1), lists["only_1"], kw["base_1"], 1.5), ((b, w2), lists["only_2"], kw["base_2"], -0.5)):
        ids, coefs = zip(*merged(only))
        want, want_w = hl.brownian_bridge(shape, "cuda", ids, coefs, 77, 0, None, base_a=base[0], fa=base[1], base_b=base[2], fb=base[3], prev=prev,
                                          scale=scale)
        assert torch.equal(out, want) and torch.equal(w, want_w)


def test_fallbacks_are_the_two_calls(api, monkeypatch):
    ng, hl = api.noise_generation, api.hl
    x = torch.zeros((1, 4, 16, 16), device="cuda")
    mk = lambda depth=24: tuple(ng.BrownianTreeNoiseSampler(x, LO, HI, seed=9, tree_depth=depth) for _ in range(2))  # noqa: E731
    calls = counted(monkeypatch, hl)

    def same(one, two, s, sm, sn):
        a, b = one.pair(s, sm, sn)
        assert torch.equal(a, two(s, sm)) and torch.equal(b, two(s, sn))
        assert list(one._points) == list(two._points)

    one, two = mk()
    one(9.0, 5.0), two(9.0, 5.0)
    same(one, two, 9.0, 7.0, 5.0)       # the second time is kept already
    same(one, two, 9.0, 5.0, 7.0)       # ... both are
    same(one, two, 9.0, 3.5, 3.5)       # both queries ask for the same time
    same(*mk(), LO, 5.0, 9.0)           # from t_lo (W = 0, nothing to difference against): one launch, no prev
    same(*mk(), HI, 9.0, 5.0)           # W(sigma) not kept (a run's first step), no statistics asked for: evaluated first, then one launch
    same(*mk(), 9.0, 5.0, LO)           # W(sigma) not kept and a query for t_lo: scale * W(sigma), W(t_lo) is not evaluated
    same(*mk(0), 9.0, 7.0, 5.0)         # the path of bridges: the second point hangs on the first
    assert calls["pair"] == 2
    # depth 6: both times resolve to one grid point -- the second increment equals the first, its point is kept by then
    one, two = mk(6)
    cell = (HI - LO) / 64
    same(one, two, 9.0, 5.0, 5.0 + 0.2 * cell)
    # ... and a time within the grid's tolerance of sigma: the zero increment, no launch for it
    on_grid = one.path.resolve(9.0)
    a, b = one.pair(on_grid, on_grid + 0.2 * cell, 3.0)
    assert not a.any() and torch.equal(b, two(on_grid, 3.0))
    assert calls["pair"] == 2
    # the summed term count beyond what one launch takes (here: a lowered limit) -> two calls
    monkeypatch.setattr(hl, "BROWNIAN_MAX_TERMS", 30)
    same(*mk(), 9.0, 7.0, 5.0)
    assert calls["pair"] == 2
    monkeypatch.setattr(hl, "BROWNIAN_MAX_TERMS", 96)
    same(*mk(), 9.0, 7.0, 5.0)
    assert calls["pair"] == 3


def test_shards_see_their_own_global_elements(api):
    ng = api.noise_generation
    x = torch.zeros((2, 4, 32, 32), device="cuda")
    full = ng.BrownianTreeNoiseSampler(x, LO, HI, seed=4, tree_depth=24)
    with ng.shard_offset(1):
        part = ng.BrownianTreeNoiseSampler(x[:1], LO, HI, seed=4, tree_depth=24)
    for s, s_next in zip(SCHEDULE[:3], SCHEDULE[1:]):
        a, b = full.pair(s, mid(s, s_next), s_next)
        pa, pb = part.pair(s, mid(s, s_next), s_next)
        assert torch.equal(a[1:], pa) and torch.equal(b[1:], pb)


def run_sampler(api, x, sigmas, **params):
    model = lambda x, sigma, **kw: 0.5 * x  # noqa: E731
    return api.sonar.SonarDPMPPSDE.sampler(model, x.clone(), sigmas, extra_args={"seed": 31}, disable=True, sonar_params=params)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_sampler_with_the_pair_is_the_sampler_without(api, monkeypatch, dtype):
    S = api.sonar.SonarDPMPPSDE
    assert S.brownian_pair is False  # (the default: one launch measured slower than the two on cfg5's shard, profiles/brownian_pair_time.txt)
    monkeypatch.setattr(S, "brownian_pair", True)
    x = torch.randn((1, 4, 32, 32), device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)).to(dtype)
    sigmas = torch.tensor([14.6, 7.0, 3.0, 1.2, 0.4], device="cuda")
    calls = counted(monkeypatch, api.hl)
    on = run_sampler(api, x, sigmas, noise_type="brownian")
    # (a normalised draw reduces statistics: the run's first and last step, which touch the ends of the range, keep their two calls --
    # test_pair_equals_two_calls_over_a_schedule says why)
    assert calls == {"pair": 2, "single": 4}, "ONE increment launch per step between the first and the last"
    monkeypatch.setattr(S, "brownian_pair", False)
    off = run_sampler(api, x, sigmas, noise_type="brownian")
    assert calls == {"pair": 2, "single": 12}, "two per step with the pair switched off"
    assert on.dtype == dtype and torch.equal(on, off)


def test_sampler_pair_through_a_one_item_chain_only(api, monkeypatch):
    N, S = api.noise, api.sonar.SonarDPMPPSDE
    x = torch.randn((1, 4, 32, 32), device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    sigmas = torch.tensor([14.6, 7.0, 3.0, 1.2, 0.4], device="cuda")

    def chain(*types_):
        c = N.CustomNoiseChain()
        for t in types_:
            c.add(N.CustomNoiseItem(0.5, noise_type=t))
        return c

    calls = counted(monkeypatch, api.hl)
    monkeypatch.setattr(S, "brownian_pair", True)
    on = run_sampler(api, x, sigmas, custom_noise=chain("brownian"))
    assert calls == {"pair": 2, "single": 4}
    two_items = run_sampler(api, x, sigmas, custom_noise=chain("brownian", "gaussian"))
    assert calls["pair"] == 2 and two_items.isfinite().all(), "a longer chain keeps its two calls"
    monkeypatch.setattr(S, "brownian_pair", False)
    single = calls["single"]
    off = run_sampler(api, x, sigmas, custom_noise=chain("brownian"))
    assert calls["pair"] == 2 and calls["single"] == single + 8 and torch.equal(on, off)


def test_other_noise_types_are_not_asked_for_a_pair(api, monkeypatch):
    ng = api.noise_generation
    asked = []

    def refuse(*a, **k):
        asked.append(a)
        raise AssertionError("a two-point query for another noise type")

    monkeypatch.setattr(ng.BrownianTreeNoiseSampler, "pair", refuse)
    monkeypatch.setattr(ng.BrownianNoiseGenerator, "pair", refuse)
    x = torch.randn((1, 4, 32, 32), device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    sigmas = torch.tensor([14.6, 7.0, 3.0, 1.2, 0.4], device="cuda")
    ns = api.noise.get_noise_sampler("gaussian", x, 0.4, 14.6, seed=31, cpu=True, normalized=True)
    assert getattr(ns, "deferred_pair", None) is None, "a Gaussian sampler exposes no two-point query"
    torch.manual_seed(5)
    monkeypatch.setattr(api.sonar.SonarDPMPPSDE, "brownian_pair", True)
    out = run_sampler(api, x, sigmas, noise_type="gaussian")
    torch.manual_seed(5)
    monkeypatch.setattr(api.sonar.SonarDPMPPSDE, "brownian_pair", False)
    assert torch.equal(out, run_sampler(api, x, sigmas, noise_type="gaussian")) and not asked


def test_refusals_through_the_c_abi(api):
    """out_1 == out_2, a NULL output and an over-long term list come back with their codes and launch nothing (the tensors stay as they were)."""
    hl = api.hl
    lib = hl.load()
    o1, o2 = torch.full((4096,), 7.0, device="cuda"), torch.full((4096,), 7.0, device="cuda")
    ids = (hl.C.c_uint64 * 97)(*range(100, 197))
    cfs = (hl.C.c_float * 97)(*([0.1] * 97))

    def call(out_1, out_2, n_1=2):
        return lib.sonar_brownian_pair_f32(out_1, out_2, None, None, None, 1.0, 1.0, None, 0.0, None, 0.0, None, 0.0, None, 0.0, 4096, 0, None, None, 0,
                                           ids, cfs, n_1, ids, cfs, 2, 5, None, 4096, None, None, torch.cuda.current_stream().cuda_stream)

    assert call(o1.data_ptr(), o1.data_ptr()) == -1 and call(None, o2.data_ptr()) == -1 and call(o1.data_ptr(), None) == -1
    assert call(o1.data_ptr(), o2.data_ptr(), n_1=97) == -2
    torch.cuda.synchronize()
    assert (o1 == 7.0).all() and (o2 == 7.0).all()
    assert call(o1.data_ptr(), o2.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and abs(o1.std().item() - 0.1 * math.sqrt(2)) < 0.02
