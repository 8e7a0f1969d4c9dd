"""GPU: utils.elementwise_shuffle_by_dim and ShuffledNoise (csrc/shuffle.hip).

Replay mode against the reference's own outputs (tests/golden/shuffle.npz, written by make_shuffle_golden.py on the CPU): a shuffle is a
gather, every output value is an input value, so the comparison is torch.equal -- and the host generator must stand where the reference's
stands after the call.  Generate mode against the host restatement of its stream contract (tests/shuffle_refs.py), torch.equal again, on
inputs of distinct values.  The item over a gaussian base goes through scale_noise first: the chain tolerance of the node sweep
(rtol = 4e-5, atol = 4e-5 * max(1, peak))."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import shuffle_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import shuffle_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, STREAM = 2**32 + 5, 2**33 + 9


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def shuffle(nz):
    return nz.utils.elementwise_shuffle_by_dim


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "shuffle.npz"), allow_pickle=False)


def planted(shape, dtype=torch.float32):
    return torch.arange(int(np.prod(shape)), dtype=dtype).reshape(shape)


def _rng(kind):
    if kind == "gen":
        return torch.Generator().manual_seed(cases.SEED)
    torch.manual_seed(cases.SEED)
    return None


# ------------------------------------------------------------------------------------------------ 1. replay mode against the reference
@pytest.mark.parametrize("case", list(cases.replay_cases()), ids=lambda c: c[0])
def test_replay_equals_the_reference(shuffle, g, case):
    name, shape, dim, prob, no_identity, rng = case
    x = torch.from_numpy(g[f"in_{'x'.join(map(str, shape))}"]).to(DEV)
    before = x.clone()
    gen = _rng(rng)
    out = shuffle(x, dim=dim, prob=prob, no_identity=no_identity, generator=gen)
    after = torch.rand(4, generator=gen)
    assert out.is_cuda and out.dtype == torch.float32 and out.data_ptr() != x.data_ptr() and torch.equal(x, before)
    assert torch.equal(out.cpu(), torch.from_numpy(g[f"out_{name}"]))
    assert torch.equal(after, torch.from_numpy(g[f"next_{name}"])), "the host generator is not where the reference leaves it"


def test_replay_half_precision(shuffle, g):
    shape, dim, prob, no_identity = cases.HALF_CASE
    gen = _rng("global")
    out = shuffle(planted(shape, torch.float16).to(DEV), dim=dim, prob=prob, no_identity=no_identity)
    assert out.dtype == torch.float16 and torch.equal(out.cpu(), torch.from_numpy(g["out_half"]))
    assert torch.equal(torch.rand(4, generator=gen), torch.from_numpy(g["next_half"]))


# ------------------------------------------------------------------------------------------------ 2. generate mode against the restatement
def _generate_layouts(max_n):
    yield from cases.LAYOUTS
    yield (1, 1, 1, max_n), -1
    yield (1, max_n, 2, 3), 1


def test_generate_equals_the_host_restatement(pkg, shuffle):
    for shape, dim in _generate_layouts(pkg.hip_lib.SHUFFLE_MAX_N):
        x = planted(shape)
        xd = x.to(DEV)
        for prob in (1.0, 0.5):
            for no_identity in (False, True):
                if no_identity and shape[dim] < 2:
                    continue
                out = shuffle(xd, dim=dim, prob=prob, no_identity=no_identity, device_key=(SEED, STREAM))
                want = R.shuffled(x.numpy(), dim, prob, no_identity, SEED, STREAM)
                assert torch.equal(out.cpu(), torch.from_numpy(want)), (shape, dim, prob, no_identity)
    assert torch.equal(shuffle(xd, dim=1, prob=0.0, device_key=(SEED, STREAM)), xd)
    # a negative seed is its 64-bit pattern; fp16 goes through fp32 and back
    x = planted((2, 3, 5, 7))
    out = shuffle(x.to(DEV).half(), dim=2, device_key=(-3, 4))
    assert out.dtype == torch.float16 and torch.equal(out.float().cpu(), torch.from_numpy(R.shuffled(x.numpy(), 2, 1.0, False, -3, 4)))


def test_generate_refuses_a_longer_dimension(pkg, shuffle):
    n = pkg.hip_lib.SHUFFLE_MAX_N + 1
    x = planted((2, n)).to(DEV)
    with pytest.raises(NotImplementedError, match=rf"SHUFFLE_MAX_N = {n - 1}.*use cpu noise"):
        shuffle(x, dim=1, device_key=(SEED, STREAM))
    # replay mode has no bound, and neither has a rotation (no sort keys)
    torch.manual_seed(3)
    out = shuffle(x, dim=1)
    assert torch.equal(out.sort(dim=1).values, x) and not torch.equal(out, x)
    rot = shuffle(x, dim=1, no_identity=True, device_key=(SEED, STREAM))
    assert torch.equal(rot.cpu(), torch.from_numpy(R.shuffled(x.cpu().numpy(), 1, 1.0, True, SEED, STREAM)))


# ------------------------------------------------------------------------------------------------ 3. structure, generate mode
def test_generate_structure(nz, shuffle):
    shape = (4, 3, 5, 7)
    x = planted(shape).to(DEV)
    for dim in range(4):
        n = shape[dim]
        rows_in = x.movedim(dim, -1).reshape(-1, n)
        out = shuffle(x, dim=dim, prob=0.5, device_key=(SEED, STREAM))
        assert torch.equal(out.movedim(dim, -1).reshape(-1, n).sort(dim=1).values, rows_in)  # arange rows are sorted already
        rot = shuffle(x, dim=dim, prob=0.5, no_identity=True, device_key=(SEED, STREAM)).movedim(dim, -1).reshape(-1, n)
        moved = (rot != rows_in).any(dim=1)
        assert 0 < int(moved.sum()) < moved.numel()
        for r in torch.nonzero(moved).flatten().tolist():  # a masked row is a cyclic shift by a non-zero offset
            off = int((rows_in[r] == rot[r, 0]).nonzero()) % n
            assert off != 0 and torch.equal(rot[r], torch.roll(rows_in[r], -off))
        assert torch.equal(shuffle(x, dim=dim, prob=0.5, device_key=(SEED, STREAM)), out)     # the same seed, the same bits
        assert not torch.equal(shuffle(x, dim=dim, prob=0.5, device_key=(SEED + 1, STREAM)), out)
    # two shards under shard_offset concatenate to the unsharded result
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    for dim, kw in ((-1, {}), (1, {}), (2, dict(no_identity=True, prob=0.5))):
        whole = shuffle(x, dim=dim, device_key=(SEED, STREAM), **kw)
        parts = []
        for first, count in ((0, 1), (1, 3)):
            with ng.shard_offset(first):
                parts.append(shuffle(x[first:first + count].contiguous(), dim=dim, device_key=(SEED, STREAM), **kw))
        assert torch.equal(torch.cat(parts), whole)
    with ng.shard_offset(1), pytest.raises(NotImplementedError):
        shuffle(x[1:].contiguous(), dim=0, device_key=(SEED, STREAM))


class _Fixed:
    """A chain stand-in that serves one tensor."""

    def __init__(self, t):
        self.t = t

    def clone(self):
        return self

    def make_noise_sampler(self, *a, **k):
        return lambda s, sn: self.t.clone()


def test_two_dims_entries_of_one_call_use_different_permutations(nz):
    base = planted((1, 2, 16, 16))
    item = nz.ShuffledNoise(1.0, noise=_Fixed(base.to(DEV)), dims=(-1, -2, -1), percentages=(1.0,), no_identity=False, fork_rng=False)
    ns = item.make_noise_sampler(base.to(DEV), 0.03, 14.6, seed=77, cpu=False, normalized=False)
    sig = (torch.tensor(10.0), torch.tensor(5.0))
    for call in range(2):  # entry i of call c: streams 3 (3 c + i) ..
        want = base.numpy()
        for i, dim in enumerate((-1, -2, -1)):
            want = R.shuffled(want, dim, 1.0, False, 77, 3 * (3 * call + i))
        assert torch.equal(ns(*sig).cpu(), torch.from_numpy(want))
    # entries 0 and 2 shuffle the same dimension: were they to share a stream, every row would be permuted the same way twice
    assert all(R.row_sources(77, 0, r, 16, 1.0, False) != R.row_sources(77, 6, r, 16, 1.0, False) for r in range(32))


# ------------------------------------------------------------------------------------------------ 4. the item, replay mode
def test_item_replay_equals_the_reference_item(nz, g):
    it = cases.ITEM
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.ShuffledNoise(it["factor"], noise=chain, dims=it["dims"], percentages=it["percentages"], no_identity=it["no_identity"],
                            fork_rng=it["fork_rng"]).clone()
    torch.manual_seed(it["global_seed"])
    ns = item.make_noise_sampler(torch.zeros(it["latent"], device=DEV), it["sigma_min"], it["sigma_max"], seed=it["seed"], cpu=True, normalized=True)
    want = torch.from_numpy(g["item_out"])
    for i, (s, sn) in enumerate(it["sigmas"]):
        got = ns(torch.tensor(s), torch.tensor(sn))
        assert got.is_cuda and tuple(got.shape) == tuple(want[i].shape)
        torch.testing.assert_close(got.cpu(), want[i], rtol=4e-5, atol=4e-5 * max(1.0, float(want[i].abs().max())))
    assert torch.equal(torch.rand(4), torch.from_numpy(g["item_next"]))


def test_fork_rng_leaves_the_host_generator_alone(nz):
    base = planted((1, 2, 8, 8)).to(DEV)
    item = nz.ShuffledNoise(1.0, noise=_Fixed(base), dims=(-1,), percentages=(0.5,), no_identity=False, fork_rng=True)
    ns = item.make_noise_sampler(base, 0.03, 14.6, seed=1, cpu=True, normalized=False)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    out = ns(torch.tensor(10.0), torch.tensor(5.0))
    assert torch.equal(torch.get_rng_state(), state) and not torch.equal(out, base)


# ------------------------------------------------------------------------------------------------ 5. refusals, before any launch
def test_refusals_leave_the_output_untouched(pkg):
    hl = pkg.hip_lib
    lib = hl.load()
    x = planted((2, 3, 5, 7)).to(DEV)
    out = torch.full_like(x, -1.0)
    idx = torch.zeros(30, 7, dtype=torch.int32, device=DEV)
    off = torch.ones(30, dtype=torch.int32, device=DEV)
    st = hl._stream()
    shape = (4, 2, 3, 5, 7, 1)
    px, po, pi = x.data_ptr(), out.data_ptr(), idx.data_ptr()

    def refused(fn, *args):
        with pytest.raises(hl.SonarHipError):
            hl._check(fn(*args), "shuffle")

    gather, generate = lib.sonar_shuffle_gather_f32, lib.sonar_shuffle_generate_f32
    key = (1.0, 0, 1, 2, 0, st)
    for bad in ((None, po), (px, None), (px, px)):                                        # a null pointer, out == src
        refused(gather, *bad, *shape, 3, pi, 0, st)
        refused(generate, *bad, *shape, 3, *key)
    refused(gather, px, po, *shape, 3, None, 0, st)
    for dim in (-1, 4, 5):                                                                # dim out of range
        refused(gather, px, po, *shape, dim, pi, 0, st)
        refused(generate, px, po, *shape, dim, *key)
    refused(gather, px, po, 4, 2, 3, 0, 7, 1, 2, pi, 0, st)                               # n < 1
    refused(generate, px, po, 4, 2, 3, 0, 7, 1, 2, *key)
    refused(gather, px, po, 4, 210, 1, 1, 1, 1, 1, off.data_ptr(), 1, st)                 # n < 2 with offsets
    refused(generate, px, po, 4, 210, 1, 1, 1, 1, 1, 1.0, 1, 1, 2, 0, st)
    refused(gather, px, po, 3, 1 << 16, 2, (1 << 15) + 1, 1, 1, 1, pi, 0, st)             # more than 2^31 rows
    refused(generate, px, po, 3, 1 << 16, 2, (1 << 15) + 1, 1, 1, 1, *key)
    with pytest.raises(hl.SonarHipError):
        hl.shuffle_gather(x, 3, idx, offsets=False, out=x)
    with pytest.raises(hl.SonarHipError):
        hl.shuffle_generate(x, 4, 1.0, False, 1, 2, out=out)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    # rows == 0 launches nothing and succeeds
    assert lib.sonar_shuffle_generate_f32(px, po, 4, 2, 0, 5, 7, 1, 3, *key) == 0 and lib.sonar_shuffle_gather_f32(px, po, 4, 2, 0, 5, 7, 1, 3, pi, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
