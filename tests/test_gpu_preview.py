"""-m gpu: the filter previews of SonarPowerNoise / SonarPowerFilterNoise, composed by csrc/preview.hip, against the reference's pictures
(tests/golden/preview.npz, tests/golden/make_preview_golden.py).

Raw fp32 panels: the tolerance the spectral filter has against its goldens (``near`` of tests/test_gpu_round2.py: 2e-5 of the reference's
peak) -- the kernel panel is an irfft2 on that path, the filter panel is elementwise.

uint8 images: the cast truncates, so a value within rounding of a whole number may land on either side.  Every pixel within one grey level
of the reference's, at most 2 % of the pixels different at all, shapes equal.  The cap is a condition on the cases, not a measured
tolerance: the generator stores a case only if the reference's own fp32 picture against an fp64 evaluation of the same formulas differs in
fewer than 1 % of its pixels, none by more than one level.  Observed there: 0 % in all 38 stored cases (worst level difference 0); the
default band-pass on the 6 x 10 plane had 14.5 % (45 % of its kernel panel: exact zeros around the spike in fp64, +-1e-8 in fp32, grey
level 128 or 127) and was replaced by the band-pass 0.1 .. 0.35.  Observed here, on an MI355X: no pixel differs in any case (the device's
transforms return exact zeros around an all-pass filter's spike too, up to 1.4e-7 in a few places of the 7 x 9 and 9 x 7 planes); raw
panels within 1.8e-7 of the reference's peak."""
import importlib
import json
import os
import random
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))
META = json.loads(str(np.load(os.path.join(GOLDEN, "preview.npz"), allow_pickle=False)["meta_json"]))
CASES, FILTERS = META["cases"], META["filters"]
SMALL = [tuple(s) for s in META["small"]]


@pytest.fixture(scope="module")
def pn(pkg):
    pkg.hip_lib.load()
    return importlib.import_module("comfyui_sonar_amd.py.nodes.powernoise")


@pytest.fixture(scope="module")
def g(golden):
    return golden("preview")


def near(a, b, rel=2e-5):
    b = b.detach().cpu().float()
    torch.testing.assert_close(a.detach().cpu().float(), b, rtol=0, atol=rel * float(b.abs().max()))


def check_image(got, want, name=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (name, got.shape, want.shape)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float((diff != 0).mean())
    print(f"{name}: {share:.4%} of the pixels differ, worst {int(diff.max())}")
    assert diff.max() <= 1, f"{name}: a pixel is {int(diff.max())} grey levels off"
    assert share <= 0.02, f"{name}: {share:.2%} of the pixels differ"


def rng_position():
    """Seed, Philox offset and state bytes of the current device's default generator: what DeviceRNG hands stream ids out of."""
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset(), bytes(torch.cuda.get_rng_state().tolist())


def make_filter(pn, spec):
    spec = dict(spec)
    inner = spec.pop("compose_with", None)
    return pn.PowerFilter(compose_with=None if inner is None else pn.PowerFilter(**inner), **spec)


def node_sockets(key, **over):
    kw = {k: v["default"] for k, v in ABI[key]["inputs"].items() if "default" in v}
    kw.pop("preview", None)
    return dict(kw, **over)


def item_for(pn, case):
    if case["filter"] == "node":
        return pn.PowerNoiseItem(**node_sockets("SonarPowerNoise", mix=case["mix"]))
    return pn.PowerNoiseItem(1.0, power_filter=make_filter(pn, FILTERS[case["filter"]]), time_brownian=False, mix=case["mix"], common_mode=0.0,
                             channel_correlation="1, 1, 1, 1, 1, 1", filter_norm_factor=case["norm"])


# ------------------------------------------------------------------------------------------------ the reference's pictures
@pytest.mark.parametrize("name", sorted(CASES))
def test_raw_panels_match_the_reference(pn, g, name):
    case = CASES[name]
    item = item_for(pn, case)
    nf = getattr(item, "filter_norm_factor", 1.0)
    got_f, got_k = item.power_filter.preview(size=tuple(case["size"]), mix=case["mix"], normalization_factor=nf, raw=True)
    want_f, want_k = g[f"{name}/filter_panel"], g[f"{name}/kernel_panel"]
    assert got_f.is_cuda and got_f.dtype == torch.float32 and tuple(got_f.shape) == tuple(want_f.shape)
    assert tuple(got_k.shape) == tuple(want_k.shape)
    near(got_f, want_f)
    near(got_k, want_k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_matches_the_reference(pkg, pn, g, name, monkeypatch):
    case = CASES[name]
    spectra, irfft2 = [], pkg.hip_lib.power_irfft2

    def spy(z, *args, **kw):  # the spectra the preview hands to the inverse transform: ones (kernel plane) and the host draw
        spectra.append(z.cpu())
        return irfft2(z, *args, **kw)

    monkeypatch.setattr(pkg.hip_lib, "power_irfft2", spy)
    state, pystate = torch.random.get_rng_state(), random.getstate()
    dev = rng_position()
    img = item_for(pn, case).preview(size=tuple(case["size"]))
    assert img.mode == "L"
    check_image(img, g[f"{name}/image"], name)
    assert torch.equal(torch.random.get_rng_state(), state) and random.getstate() == pystate, "the preview moved a global RNG"
    assert rng_position() == dev, "the preview moved the device generator"
    drawn = [z for z in spectra if not torch.equal(z, torch.ones_like(z))]
    assert len(spectra) == 2 and len(drawn) == 1 and torch.equal(drawn[0], g[f"{name}/spectrum"]), "the sample is not the reference's seed-0 draw"


@pytest.mark.parametrize("name", ["16x12_shaped_m1.0_n1.0", "8x6_composed_m1.0_n0.5"])
def test_two_panel_image_is_the_raw_panels_truncated(pn, g, name):
    """PowerFilter.preview(raw=False): the ``L`` image of the two panels, against the reference's raw panels clamped and cast."""
    case = CASES[name]
    filt = make_filter(pn, FILTERS[case["filter"]])
    img = filt.preview(size=tuple(case["size"]), mix=case["mix"], normalization_factor=case["norm"])
    want = torch.cat((g[f"{name}/filter_panel"], g[f"{name}/kernel_panel"]), dim=-1).clamp(0, 255).to(torch.uint8)[0, 0].numpy()
    assert img.mode == "L"
    check_image(img, want, name)


@pytest.mark.parametrize("size", SMALL)
def test_rfft2_to_fft2_is_bit_equal(pn, g, size):
    h, w = size
    x = g[f"fft2/{h}x{w}/in"].cuda()
    before = x.clone()
    out = pn.rfft2_to_fft2(x)
    assert out.is_cuda and tuple(out.shape) == (1, 2, h, 2 * (w // 2 + 1) - (2 if (w // 2 + 1) % 2 else 1))
    assert torch.equal(out.cpu(), g[f"fft2/{h}x{w}/out"]) and torch.equal(x, before)


def test_raw_entry_point_without_gain_moves_data_only(pkg, pn):
    """gain=False with all three planes: F, the rolled kernel and the noise, bit for bit (three planes, a width that is no multiple of 4)."""
    hl = pkg.hip_lib
    gen = torch.Generator().manual_seed(3)
    h, w = 7, 10
    filt, kern, noise = (torch.randn((3, h, n), generator=gen) for n in (w // 2 + 1, w, w))
    out = hl.preview_panels(filt.cuda(), kern.cuda(), noise.cuda(), w, gain=False).cpu()
    x_r = filt.roll(h // 2, -2)
    x_l = torch.flip(x_r[..., 1:None], dims=(-2, -1))  # Wh = 6, even: only column 0 dropped; H odd: no extra roll
    want = torch.cat((x_l, x_r, kern.roll((h // 2, w // 2), (-2, -1)), noise), dim=-1)
    assert tuple(out.shape) == (3, h, 11 + 2 * w) and torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ the nodes
@pytest.fixture()
def temp_folder(tmp_path, monkeypatch):
    """A stand-in folder_paths that saves into tmp_path."""
    monkeypatch.setitem(sys.modules, "folder_paths", types.SimpleNamespace(
        get_temp_directory=lambda: str(tmp_path), get_save_image_path=lambda prefix, directory: (directory, prefix, 0, "", prefix)))
    return str(tmp_path)


def draw(chain, seed=1):
    x = torch.zeros((1, 4, 32, 32), device="cuda")
    torch.manual_seed(seed)
    return chain.make_noise_sampler(x, 0.03, 14.6, seed=seed, cpu=True, normalized=True)(torch.tensor(14.6), torch.tensor(10.0))


def check_node_result(out, folder):
    assert isinstance(out, dict) and set(out) == {"ui", "result"} and isinstance(out["result"], tuple) and len(out["result"]) == 1
    (entry,) = out["ui"]["images"]
    assert entry["type"] == "temp" and entry["subfolder"] == "" and entry["filename"].startswith("sonar_temp_")
    path = os.path.join(folder, entry["filename"])
    with Image.open(path) as img:
        img.load()
    return img


@pytest.mark.parametrize("preview,mix,golden_case", [("mix", 1.0, "128x128_node_m1.0_n1.0"), ("mix", 0.5, "128x128_node_m0.5_n1.0"),
                                                     ("no_mix", 0.5, "128x128_node_m1.0_n1.0")])
def test_power_noise_node_preview(pkg, g, temp_folder, preview, mix, golden_case):
    node = pkg.NODE_CLASS_MAPPINGS["SonarPowerNoise"]
    kw = node_sockets("SonarPowerNoise", mix=mix)
    state, pystate = torch.random.get_rng_state(), random.getstate()
    out = node().go(preview=preview, **kw)
    assert torch.equal(torch.random.get_rng_state(), state) and random.getstate() == pystate
    img = check_node_result(out, temp_folder)
    assert img.mode == "L"
    check_image(img, g[f"{golden_case}/image"], f"{preview}/{mix}")
    plain = node().go(preview="none", **kw)
    assert isinstance(plain, tuple) and out["result"][0].items[0].mix == mix  # "no_mix" changes the picture's item only
    assert torch.equal(draw(out["result"][0]), draw(plain[0]))


def test_power_filter_noise_node_preview(pkg, g, temp_folder):
    M = pkg.NODE_CLASS_MAPPINGS
    nz = importlib.import_module("comfyui_sonar_amd.py.noise")
    inner = nz.CustomNoiseChain()
    inner.add(nz.CustomNoiseItem(1.0, noise_type=nz.NoiseType.GAUSSIAN))
    (filt,) = M["SonarPowerFilter"].go(compose_mode="max", **node_sockets("SonarPowerFilter"))
    kw = dict(node_sockets("SonarPowerFilterNoise"), sonar_custom_noise=inner, sonar_power_filter=filt, normalize_result="default",
              normalize_noise="default")
    out = M["SonarPowerFilterNoise"]().go(preview="mix", **kw)
    img = check_node_result(out, temp_folder)
    assert img.mode == "L"
    check_image(img, g["128x128_node_m1.0_n1.0/image"], "filter-noise mix")  # the filter node's default sockets are PowerNoise's
    plain = M["SonarPowerFilterNoise"]().go(preview="none", **kw)
    assert torch.equal(draw(out["result"][0]), draw(plain[0]))


def filter_noise_item(pn, **over):
    nz = importlib.import_module("comfyui_sonar_amd.py.noise")
    inner = nz.CustomNoiseChain()
    inner.add(nz.CustomNoiseItem(1.0, noise_type=nz.NoiseType.GAUSSIAN))
    kw = dict(noise=inner, normalize_noise=None, normalize_result=None, power_filter=pn.PowerFilter(alpha=1.0), mix=1.0, common_mode=0.0,
              channel_correlation="1, 1, 1, 1, 1, 1", time_brownian=True, filter_norm_factor=1.0)
    return pn.PowerFilterNoiseItem(1.0, **dict(kw, **over))


def test_custom_preview_without_comfyui_is_refused(pn, monkeypatch):
    monkeypatch.setitem(sys.modules, "latent_preview", None)
    with pytest.raises(NotImplementedError, match="latent_preview"):
        filter_noise_item(pn, preview_type="custom").preview()


@pytest.fixture()
def rng_restored():
    """The test reseeds torch's generators: they go back to where the suite had them."""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        yield


def test_custom_preview_pastes_the_colour_panel(pkg, pn, temp_folder, monkeypatch, rng_restored):
    colour, seen = (200, 30, 90), []

    class Previewer:
        def decode_latent_to_preview(self, latent):
            seen.append(latent)
            return Image.new("RGB", (16, 16), colour)

    monkeypatch.setitem(sys.modules, "latent_preview", types.SimpleNamespace(get_previewer=lambda device, fmt: Previewer()))
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    torch.cuda.manual_seed(987654321)  # a position of the device generator that is not seed 0, offset 0: a reseed would show
    ng.DeviceRNG.take(3)
    state, pystate, dev = torch.random.get_rng_state(), random.getstate(), rng_position()
    assert dev[:2] == (987654321, 12)
    img = filter_noise_item(pn, preview_type="custom").preview()
    assert torch.equal(torch.random.get_rng_state(), state) and random.getstate() == pystate
    assert rng_position() == dev, "the custom preview moved the device generator"
    assert ng.DeviceRNG.take(1) == (987654321, 3) and ng.DeviceRNG.rewind(3, 1)  # the next stream id is the one that was due
    assert img.mode == "RGB" and img.size == (3 * 128, 128)
    px = np.asarray(img)
    assert (px[:, 256:] == np.array(colour, dtype=np.uint8)).all(), "the previewer's colour must fill the third panel"
    grey = np.asarray(filter_noise_item(pn).preview())
    assert (px[:, :256] == grey[:, :256, None]).all()  # the first two panels are the grey preview's
    (latent,) = seen
    assert not latent.is_cuda and tuple(latent.shape) == (1, 4, 128, 128) and bool(torch.isfinite(latent).all()) and float(latent.std()) > 0.1
    # through the node, as a graph does it
    M = pkg.NODE_CLASS_MAPPINGS
    (filt,) = M["SonarPowerFilter"].go(compose_mode="max", **node_sockets("SonarPowerFilter"))
    out = M["SonarPowerFilterNoise"]().go(preview="custom", **dict(node_sockets("SonarPowerFilterNoise"), sonar_custom_noise=filter_noise_item(pn).noise,
                                                                    sonar_power_filter=filt, normalize_result="default", normalize_noise="default"))
    assert check_node_result(out, temp_folder).mode == "RGB"
    assert torch.equal(torch.random.get_rng_state(), state) and random.getstate() == pystate and rng_position() == dev, "the node moved a generator"
    # the picture does not depend on where the generators stood
    torch.manual_seed(5)
    again = np.asarray(filter_noise_item(pn, preview_type="custom").preview())
    assert np.array_equal(again, px)


# ------------------------------------------------------------------------------------------------ a caller's noise, refusals
def test_a_supplied_noise_tensor_is_left_alone(pkg, pn, g):
    name = "16x12_shaped_m1.0_n1.0"
    item = item_for(pn, CASES[name])
    noise = torch.randn((1, 1, 16, 12), generator=torch.Generator().manual_seed(9)).cuda()
    before = noise.clone()
    img = np.asarray(item.preview(size=(16, 12), noise=noise))
    assert torch.equal(noise, before), "the caller's tensor was modified"
    want = np.asarray(g[f"{name}/image"])
    assert img.shape == want.shape
    fw = img.shape[1] - 2 * 12
    check_image(img[:, :fw + 12], want[:, :fw + 12], "filter and kernel panels")  # the first two panels do not depend on the noise
    # the third: the reference's own steps on the host (py/nodes/powernoise.py:430-435, 447), independent of the device's transforms
    filt = item.make_filter((16, 12), oversample=1)
    sample = torch.fft.irfft2(torch.fft.rfft2(before.cpu(), norm="ortho") * filt, s=(16, 12), norm="ortho")
    check_image(img[:, fw + 12:], ((sample * (1 / 3)).tanh() + 1.0).mul(128.0).clamp(0, 255).to(torch.uint8)[0, 0].numpy(), "noise panel")
    host = torch.randn((1, 1, 16, 12), generator=torch.Generator().manual_seed(9))
    assert np.array_equal(np.asarray(item.preview(size=(16, 12), noise=host)), img) and torch.equal(host.cuda(), before)
    with pytest.raises(ValueError):
        item.preview(size=(16, 12), noise=torch.zeros((1, 1, 12, 16), device="cuda"))


def test_entry_points_refuse_bad_arguments(pkg):
    hl = pkg.hip_lib
    lib = hl.load()
    h, w = 8, 6
    filt, kern, noise = (torch.ones((h, n), device="cuda") for n in (w // 2 + 1, w, w))
    out32 = torch.full((h, 7 + 2 * w), -7.0, device="cuda")
    out8 = torch.full((h, 7 + 2 * w), 77, dtype=torch.uint8, device="cuda")
    f, k, n = filt.data_ptr(), kern.data_ptr(), noise.data_ptr()
    bad = [  # (filter, kernel, noise, planes, H, W, noise_h, noise_w)
        (None, k, n, 1, h, w, h, w), (f, None, n, 1, h, w, h, w), (f, None, None, 1, h, w, 0, 0), (f, k, n, 1, 1, w, 1, w), (f, k, n, 1, h, 1, h, 1),
        (f, k, n, 1, h, w, h, w + 2), (f, k, n, 1, h, w, h - 1, w), (f, k, n, 1, h, w, 0, 0), (f, k, None, 1, h, w, h, w), (f, k, n, 0, h, w, h, w),
    ]
    for args in bad:
        assert lib.sonar_preview_panels_f32(*args, 1 / 3, 1 / 3, 1, out32.data_ptr(), None) == hl.ERR_ARG, args
        assert lib.sonar_preview_compose_u8(*args, 1 / 3, 1 / 3, out8.data_ptr(), None) == hl.ERR_ARG, args
    assert lib.sonar_preview_panels_f32(f, k, n, 1, h, w, h, w, 1 / 3, 1 / 3, 1, None, None) == hl.ERR_ARG
    assert lib.sonar_preview_compose_u8(f, k, n, 1, h, w, h, w, 1 / 3, 1 / 3, None, None) == hl.ERR_ARG
    assert lib.sonar_preview_panels_f32(f, None, n, 1, h, w, h, w, 1 / 3, 1 / 3, 0, out32.data_ptr(), None) == hl.ERR_ARG  # noise needs the kernel plane
    torch.cuda.synchronize()
    assert bool((out32 == -7.0).all()) and bool((out8 == 77).all()), "a refused call launched"
    # the binding: wrong shapes and a missing kernel plane raise
    with pytest.raises(hl.SonarHipError):
        hl.preview_compose(filt, None, None, w)
    with pytest.raises(hl.SonarHipError):
        hl.preview_panels(filt, kern, torch.ones((h, w + 2), device="cuda"), w)
    with pytest.raises(hl.SonarHipError):
        hl.preview_panels(filt, torch.ones((h + 1, w), device="cuda"), None, w)
    with pytest.raises(hl.SonarHipError):
        hl.preview_panels(filt.cpu(), kern, None, w)
