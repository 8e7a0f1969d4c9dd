"""-m gpu: SonarNoiseImage on the device.

Fixture cases (tests/golden/image_noise.npz, the reference's node run in replay mode) go through NODE_CLASS_MAPPINGS["SonarNoiseImage"] with
the image on the host.  Tolerance: the one tests/test_gpu_host_api.py uses for the same noise types through the sampler API (rtol 2e-5,
atol 5e-6) -- the chain after the noise (range rescale, multiplier, blend, clip / rescale) is the reference's operation sequence value for
value, so it adds nothing of its own; every noise type also has a rescale-mode case, where no clip can hide an error.

Compose-kernel parity: hip_lib.image_noise_compose on a supplied noise tensor against the same steps as plain torch calls on the CPU, bit
for bit in both overflow modes, with and without the greyscale fold.

Generate mode (cpu_noise=False) has no reference values: properties only."""
import importlib
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

KEY = "SonarNoiseImage"
META = json.loads(str(np.load(os.path.join(GOLDEN, "image_noise.npz"), allow_pickle=False)["meta_json"]))["cases"]
ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))[KEY]["inputs"]
DEFAULTS = {k: v["default"] for k, v in ABI.items() if "default" in v}
DEFAULTS.update(noise_type="gaussian")


@pytest.fixture(scope="module")
def node(pkg):
    pkg.hip_lib.load()
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry").NODE_CLASS_MAPPINGS[KEY]


def run_node(node, image, seed, chain=None, **over):
    kw = dict(DEFAULTS, seed=seed, image=image, **over)
    if chain is not None:
        nz = importlib.import_module("comfyui_sonar_amd.py.noise")
        c = nz.CustomNoiseChain()
        for factor, typ in chain:
            c.add(nz.CustomNoiseItem(factor, noise_type=nz.NoiseType[typ.upper()]))
        kw["custom_noise_opt"] = c
    return node.go(**kw)[0]


# ------------------------------------------------------------------------------------------------ the reference's runs
@pytest.mark.parametrize("name", sorted(META))
def test_fixture_case(node, golden, name):
    g, m = golden("image_noise"), META[name]
    image = g[f"image_{m['image']}"]
    before = image.clone()
    torch.manual_seed(4242)
    random.seed(4242)
    st_torch, st_py = torch.random.get_rng_state(), random.getstate()
    assert m["rng_restored"] is True  # what the reference did
    if m["error"] is not None:
        with pytest.raises({"ValueError": ValueError}[m["error"]]):
            run_node(node, image, m["seed"], **m["kwargs"])
    else:
        want = g[f"out_{name}"]
        out = run_node(node, image, m["seed"], **m["kwargs"])
        assert out.device == image.device and out.dtype == image.dtype == torch.float32 and tuple(out.shape) == tuple(want.shape)
        torch.testing.assert_close(out, want, rtol=2e-5, atol=5e-6)
    assert torch.equal(image, before), "the input image was modified"
    assert torch.equal(torch.random.get_rng_state(), st_torch) and random.getstate() == st_py, "RNG state not restored"


def test_fixture_covers_what_it_should():
    kinds = {(m["kwargs"].get("noise_type", "gaussian"), m["kwargs"].get("overflow_mode", "clamp")) for m in META.values()}
    assert {(t, o) for t in ("gaussian", "perlin", "pyramid", "uniform") for o in ("clamp", "rescale")} <= kinds
    assert {m["kwargs"].get("blend_mode", "simple_add") for m in META.values()} == {"simple_add", "lerp", "inject", "subtract_b"}
    assert sum(1 for n in META if n.startswith("c4_")) == 15 and any("chain" in m["kwargs"] for m in META.values())


# ------------------------------------------------------------------------------------------------ the compose kernel against torch
def nts(t, lo, hi, dim=(-3, -2, -1), eps=1e-07):
    mn, mx = t.amin(dim=dim, keepdim=True), t.amax(dim=dim, keepdim=True)
    n = t - mn
    n /= (mx - mn).add_(eps)
    return n.mul_(hi - lo).add_(lo).clamp_(lo, hi)


BLENDS = {"simple_add": lambda a, b, _t: a + b, "lerp": torch.lerp, "inject": lambda a, b, t: (b * t).add_(a), "subtract_b": lambda a, b, t: a - b * t}


def torch_compose(noise, image, *, noise_range, multiplier, greyscale, blend, strength, targets, rescale):
    """The node's steps after scale_noise, as the torch calls the issue lists, on the CPU."""
    result = noise.clone()
    image = image.clone().movedim(-1, 1)
    if greyscale:
        result = result.mean(dim=1, keepdim=True).expand(image.shape).contiguous()
    if noise_range is not None:
        result = nts(result, *noise_range)
    result *= multiplier
    image[:, targets, ...] = BLENDS[blend](image[:, targets, ...], result[:, targets, ...], strength)
    image = nts(image, 0.0, 1.0) if rescale else image.clip_(0, 1)
    return image.movedim(1, -1).contiguous()


def device_compose(hl, noise, image, *, noise_range, multiplier, greyscale, blend, strength, targets, rescale):
    b, h, w, c = image.shape
    result = noise.cuda()
    if greyscale:
        result = hl.image_channel_mean(result)
    lo = hi = None
    if noise_range is not None:
        lo, hi = hl.minmax_rows(result, b, result.numel() // b)
    src = image.cuda()
    kept = src.clone()
    out = hl.image_noise_compose(result, src, (b, h, w, c), noise_lo=lo, noise_hi=hi, noise_min=(noise_range or (0, 0))[0],
                                 noise_max=(noise_range or (0, 0))[1], multiplier=multiplier, greyscale=greyscale, blend_mode=blend,
                                 blend_strength=strength, channel_mask=sum(1 << t for t in targets), clamp=not rescale)
    if rescale:
        out = hl.image_rescale_(*out)
    assert torch.equal(src, kept)
    return out.cpu()


SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 4, 33, 70)]  # NCHW: one value; odd sizes, one block; 2310 pixels: ten blocks with a ragged tail


@pytest.fixture(scope="module")
def compose_inputs():
    gen = torch.Generator().manual_seed(99)
    return {s: (torch.randn(s, generator=gen) * 1.3 + 0.1, torch.rand((s[0], s[2], s[3], s[1]), generator=gen)) for s in SHAPES}


@pytest.mark.parametrize("greyscale", [False, True])
@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("blend,strength", [("simple_add", 0.9), ("lerp", 0.3), ("lerp", 0.8), ("inject", 0.7), ("subtract_b", 0.25)])
@pytest.mark.parametrize("shape", SHAPES)
def test_compose_matches_torch(pkg, compose_inputs, shape, blend, strength, rescale, greyscale):
    noise, image = compose_inputs[shape]
    targets = tuple(range(shape[1]))[: max(1, shape[1] - 1)]  # the last channel of a multi-channel image is copied through
    kw = dict(noise_range=(-0.25, 0.85), multiplier=0.8, greyscale=greyscale, blend=blend, strength=strength, targets=targets, rescale=rescale)
    got, want = device_compose(pkg.hip_lib, noise, image, **kw), torch_compose(noise, image, **kw)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"max difference {(got - want).abs().max().item():.3e}"


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_compose_edges_match_torch(pkg, compose_inputs, shape, rescale):
    """A bitmask selecting nothing, the range rescale skipped, a range that is no pair of fp32 numbers, multiplier 0 and negative, and more
    than four channels' worth of strided path (two channels)."""
    noise, image = compose_inputs[shape]
    every = tuple(range(shape[1]))
    base = dict(noise_range=(0.0, 1.0), multiplier=0.5, greyscale=False, blend="simple_add", strength=0.5, targets=every, rescale=rescale)
    for over in (dict(targets=()), dict(noise_range=None), dict(noise_range=(0.1, 0.3), multiplier=1.0), dict(multiplier=0.0),
                 dict(multiplier=-0.75, blend="inject", strength=1.5), dict(targets=(), greyscale=True)):
        kw = dict(base, **over)
        got, want = device_compose(pkg.hip_lib, noise, image, **kw), torch_compose(noise, image, **kw)
        assert torch.equal(got, want), (over, (got - want).abs().max().item())
    if shape[1] == 4:  # the same planes as two images of two channels: the strided path
        n2, i2 = noise.reshape(2, 2, *shape[2:]).contiguous(), image[..., :2].repeat(2, 1, 1, 1).contiguous()
        kw = dict(base, targets=(0, 1), blend="lerp", strength=0.4)
        assert torch.equal(device_compose(pkg.hip_lib, n2, i2, **kw), torch_compose(n2, i2, **kw))


def test_compose_refuses_bad_arguments(pkg):
    hl = pkg.hip_lib
    noise = torch.zeros(1, 3, 4, 4, device="cuda")
    with pytest.raises(hl.SonarHipError):
        hl.image_noise_compose(noise, None, (1, 4, 4, 4))  # noise does not fit the image
    with pytest.raises(hl.SonarHipError):
        hl.image_noise_compose(noise, torch.zeros(1, 4, 4, 3), (1, 4, 4, 3))  # host image
    with pytest.raises(hl.SonarHipError):
        hl.image_noise_compose(noise, None, (1, 4, 4, 3), noise_lo=torch.zeros(1, device="cuda"))  # one extreme only
    with pytest.raises(KeyError):
        hl.image_noise_compose(noise, None, (1, 4, 4, 3), blend_mode="no_such_blend")


# ------------------------------------------------------------------------------------------------ generate mode
def test_generate_mode_properties(node):
    gen = torch.Generator().manual_seed(3)
    image = torch.rand((2, 40, 50, 3), generator=gen)
    for over in (dict(), dict(overflow_mode="rescale", noise_type="perlin"), dict(greyscale_mode=True, blend_mode="lerp", blend_strength=0.3)):
        a = run_node(node, image, 11, cpu_noise=False, **over)
        b = run_node(node, image, 11, cpu_noise=False, **over)
        c = run_node(node, image, 12, cpu_noise=False, **over)
        assert a.device == image.device and a.dtype == torch.float32 and a.shape == image.shape
        assert bool(torch.isfinite(a).all()) and a.min().item() >= 0.0 and a.max().item() <= 1.0
        assert torch.equal(a, b) and not torch.equal(a, c)
    pure = run_node(node, image, 11, cpu_noise=False, pure_noise_mode=True, noise_min=0.0, noise_max=1.0, noise_multiplier=1.0,
                    blend_mode="simple_add")
    flat = pure.reshape(2, -1)
    assert torch.equal(flat.amin(dim=1), torch.zeros(2))
    assert bool(((1.0 - flat.amax(dim=1)).abs() <= 1e-6).all())  # (hi - lo) / ((hi - lo) + eps): normalize_to_scale's eps


def test_device_image_stays_on_its_device(node):
    image = torch.rand((1, 9, 14, 4), device="cuda")
    before = image.clone()
    out = run_node(node, image, 5, channel_mode="RGBA")
    assert out.is_cuda and out.device == image.device and torch.equal(image, before)
    assert torch.equal(out.cpu(), run_node(node, before.cpu(), 5, channel_mode="RGBA"))


# ------------------------------------------------------------------------------------------------ dtypes
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_images_round_once(node, dtype):
    gen = torch.Generator().manual_seed(8)
    image = torch.rand((2, 9, 14, 3), generator=gen).to(dtype)
    for over in (dict(), dict(overflow_mode="rescale", blend_mode="inject", blend_strength=0.7)):
        want32 = run_node(node, image.float(), 21, **over)
        out = run_node(node, image, 21, **over)
        assert out.dtype == dtype and out.device == image.device and out.shape == image.shape
        assert torch.equal(out, want32.to(dtype))  # the fp32 result, rounded once
        name = {torch.float16: "float16", torch.bfloat16: "bfloat16"}[dtype]
        via_socket = run_node(node, image.float(), 21, dtype=name, **over)  # an fp32 image worked on in the half dtype: fp32 comes back
        assert via_socket.dtype == torch.float32 and torch.equal(via_socket, want32.to(dtype).float())


def test_float64_is_refused(node):
    with pytest.raises(NotImplementedError, match="float64"):
        run_node(node, torch.rand(1, 9, 14, 3), 1, dtype="float64")
    with pytest.raises(NotImplementedError, match="float64"):
        run_node(node, torch.rand(1, 9, 14, 3, dtype=torch.float64), 1)
