"""GPU: utils.quantile_normalize (HIP radix select + strategy kernels) against the reference's outputs and refusals
(tests/golden/quantile_filter.npz, tests/golden/make_quantile_golden.py), and against a float64 CPU restatement (tests/quantile_refs.py)
on large shapes: the register-resident rows, the re-read long rows, dim 0 and "global"."""
import importlib
import json
import zlib

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.quantile_refs import _restated

pytestmark = pytest.mark.gpu

TRANSCENDENTAL = ("tanh", "sigmoid", "sin", "cos", "atan")


def _golden():
    g = np.load(f"{GOLDEN}/quantile_filter.npz", allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def _utils():
    return importlib.import_module("comfyui_sonar_amd.py.utils")


@pytest.mark.parametrize("name", sorted(k for k, v in _golden()[1].items() if "input" in v))
def test_reference_cases(pkg, name):
    g, meta = _golden()
    m = meta[name]
    utils = _utils()
    x = torch.from_numpy(g[f"in_{m['input']}"]).cuda()
    before = x.clone()
    kw = dict(m["kwargs"])
    if m["error"] is not None:
        with pytest.raises(Exception) as exc:
            utils.quantile_normalize(x, **kw)
            torch.cuda.synchronize()
        assert type(exc.value).__name__ == m["error"], (exc.value, m.get("message"))
        return
    got = utils.quantile_normalize(x, **kw)
    torch.cuda.synchronize()
    assert torch.equal(x, before), "the input changed"
    want = torch.from_numpy(g[f"out_{name}"])
    assert got.is_cuda and tuple(got.shape) == tuple(want.shape)
    if got.data_ptr() == x.data_ptr():
        assert torch.equal(want, before.cpu())  # an early return of the same tensor
    strategy = kw.get("strategy", "clamp")
    tol = 4e-6 if strategy.startswith(TRANSCENDENTAL) or kw.get("pow_fac", 0.5) not in (0.0, 1.0, 0.5, 2.0) else 2e-6
    finite = torch.isfinite(want)
    peak = float(want[finite].abs().max()) if bool(finite.any()) else 1.0
    torch.testing.assert_close(got.cpu(), want, rtol=tol, atol=tol * max(1.0, peak), equal_nan=True)


# ------------------------------------------------------------------------------------------------ beyond the reference
BIG = [((64, 4, 128, 128), 1, True, "resident rows of 65536"), ((2, 16, 128, 128), 1, True, "a 256 Ki row"),
       ((4, 4, 128, 128), 1, True, "few resident rows"), ((3, 2, 64, 64), 1, False, "short rows along a middle dim"),
       ((8, 4, 128, 128), 0, True, "dim 0: one row of 512 Ki"), ((2, 4, 64, 64), None, False, "global")]


# the reference refuses dim=None for median / mode / scale_down (the golden cases check that refusal)
LARGE = [(shape, dim, flatten, strategy, q) for shape, dim, flatten, _ in BIG
         for strategy, q in (("clamp", 0.85), ("median", 0.8), ("mode_2dec", 0.9), ("scale_down", 0.75), ("replace_2pt", 0.7), ("clamp", -0.7),
                             ("mean", 0.8), ("scale_down", -0.6), ("median", -0.65))
         if not (dim is None and strategy in ("median", "mode_2dec", "scale_down"))]


@pytest.mark.parametrize("shape,dim,flatten,strategy,q", LARGE, ids=[f"{c[1]}-{c[2]}-{'x'.join(map(str, c[0]))}-{c[3]}-q{c[4]}" for c in LARGE])
def test_large_rows_against_restatement(pkg, shape, dim, flatten, strategy, q):
    utils = _utils()
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, dim, strategy, q)).encode()))
    x = torch.randn(shape, generator=g)
    got = utils.quantile_normalize(x.cuda(), quantile=q, dim=dim, flatten=flatten, strategy=strategy).cpu()
    want = _restated(x, q, dim, flatten, strategy)
    torch.testing.assert_close(got.double(), want, rtol=2e-6, atol=2e-6 * float(want.abs().max()))


def test_shard_refusal(pkg):
    utils = _utils()
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    x = torch.randn(2, 4, 8, 8, device="cuda")
    with ng.shard_offset(2):
        for kw in (dict(dim=0), dict(dim=None, flatten=False), dict(dim=1, strategy="replace")):
            with pytest.raises(NotImplementedError):
                utils.quantile_normalize(x, **kw)
        out = utils.quantile_normalize(x, dim=1)  # per-sample rows are unaffected by the shard
    torch.testing.assert_close(out, utils.quantile_normalize(x, dim=1))


def test_nodes_from_the_mappings(pkg):
    reg = importlib.import_module("comfyui_sonar_amd.py.nodes.registry")
    utils = _utils()
    latent_ops = importlib.import_module("comfyui_sonar_amd.py.latent_ops")
    noise = importlib.import_module("comfyui_sonar_amd.py.noise")
    x = torch.randn(2, 4, 16, 12, device="cuda")
    (op,) = reg.NODE_CLASS_MAPPINGS["SonarLatentOperationQuantileFilter"]().go(quantile=-0.6, dim="global", flatten=False, norm_power=0.75,
                                                                              norm_factor=1.2, strategy="sin_keepsign")
    assert isinstance(op, latent_ops.SonarLatentOperation)
    want = utils.quantile_normalize(x, quantile=-0.6, dim=None, flatten=False, nq_fac=1.2, pow_fac=0.75, strategy="sin_keepsign")
    torch.testing.assert_close(op(x, sigma=1.0), want, rtol=0, atol=0)
    (adv,) = reg.NODE_CLASS_MAPPINGS["SonarLatentOperationAdvanced"]().go(
        operation=op, start_sigma=-1.0, end_sigma=0.0, input_multiplier=1.0, output_multiplier=1.0, difference_multiplier=1.0,
        blend_mode="lerp", blend_strength=1.0)
    assert adv(latent=x, sigma=1.0).shape == x.shape
    (chain,) = reg.NODE_CLASS_MAPPINGS["SonarQuantileFilteredNoise"]().go(
        factor=1.0, custom_noise=noise.CustomNoiseChain(), quantile=0.85, dim="global", flatten=False, norm_factor=1.0, norm_power=0.5,
        normalize_noise=False, normalize="disabled", strategy="median")
    item = chain.items[-1]
    assert isinstance(item, noise.QuantileFilteredNoise) and item.norm_dim is None and item.strategy == "median"


def test_mode_skips_non_finite_and_empty_key_ranges(pkg):
    """A NaN, infinities and a far outlier in a row: the mode is that of the finite rounded values, and the window search does not walk the
    empty key range between them (the call returns at once)."""
    utils = _utils()
    x = torch.randn(2, 3, 40, 40)
    x[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0e6])
    got = utils.quantile_normalize(x.cuda(), quantile=0.9, dim=1, strategy="mode_1dec", pow_fac=1.0).cpu()
    for r in range(2):
        row, out = x[r].reshape(-1), got[r].reshape(-1)
        finite = torch.isfinite(row)
        mode = torch.round(row[finite], decimals=1).mode().values
        replaced = (out != row) & ~torch.isnan(row)
        assert int(replaced.sum()) > 0 and torch.all(out[replaced] == mode)
    assert torch.isnan(got[0, 0, 0, 0])


class _ReplayChain:
    """Stand-in for the inner chain: hands back recorded draws, one per call (clone_key clones the chain)."""

    def __init__(self, draws):
        self.draws = draws

    def clone(self):
        return _ReplayChain(self.draws)

    def make_noise_sampler(self, x, *args, **kwargs):
        it = iter(self.draws)
        return lambda sigma, sigma_next: next(it).clone()


@pytest.mark.parametrize("name", sorted(k for k, v in _golden()[1].items() if "sequence" in v))
def test_quantile_filtered_noise_sequences(pkg, name):
    """QuantileFilteredNoise, cloned, sampled three times over the reference's own gaussian + perlin draws: filter, then scale_noise."""
    g, meta = _golden()
    m = meta[name]
    noise = importlib.import_module("comfyui_sonar_amd.py.noise")
    raws = torch.from_numpy(g[f"{name}_raw"]).cuda()
    want = torch.from_numpy(g[f"{name}_out"])
    item = noise.QuantileFilteredNoise(m["factor"], noise=_ReplayChain(list(raws)), normalize=True, normalize_noise=False, **m["sequence"]).clone()
    ns = item.make_noise_sampler(torch.zeros(want.shape[1:], device="cuda"), 0.1, 10.0, seed=42, cpu=True, normalized=True)
    for (s, sn), w in zip(m["sigmas"], want):
        got = ns(s, sn).cpu()
        torch.testing.assert_close(got, w, rtol=4e-6, atol=4e-6 * max(1.0, float(w.abs().max())))
    assert torch.equal(raws.cpu(), torch.from_numpy(g[f"{name}_raw"]))  # the draws are not written through


def test_latent_op_inside_advanced(pkg):
    g, meta = _golden()
    kw = meta["advop"]["latent_op"]
    reg = importlib.import_module("comfyui_sonar_amd.py.nodes.registry")
    (op,) = reg.NODE_CLASS_MAPPINGS["SonarLatentOperationQuantileFilter"]().go(
        quantile=kw["quantile"], dim=str(kw["dim"]), flatten=kw["flatten"], norm_power=kw["pow_fac"], norm_factor=kw["nq_fac"], strategy=kw["strategy"])
    (adv,) = reg.NODE_CLASS_MAPPINGS["SonarLatentOperationAdvanced"]().go(
        operation=op, start_sigma=10.0, end_sigma=1.0, input_multiplier=1.2, output_multiplier=1.0, difference_multiplier=0.9,
        blend_mode="lerp", blend_strength=0.7)
    x = torch.from_numpy(g["in_base"]).cuda()
    got = adv(latent=x, sigma=torch.tensor([5.0])).cpu()
    want = torch.from_numpy(g["advop_out"])
    torch.testing.assert_close(got, want, rtol=4e-6, atol=4e-6 * max(1.0, float(want.abs().max())))
