"""CPU: the scattering layer's fp64 statement (tests/scatternet_refs.py) by its defining properties, ScatternetFilteredNoiseGenerator's window
arithmetic against hand-worked literals, every refusal at construction, the entry point declared / bound / exported, the item's
signature, clone and inner-chain request, and the unchanged registry.  pytorch_wavelets is absent: parity unpinned."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import scatternet_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def ng(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise_generation")


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


# ---- properties of the statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("biort", ["near_sym_a", "legall", "antonini"])
def test_a_constant_plane_gives_the_constant_and_no_magnitude(biort):
    z = R.scat_layer(np.full((1, 2, 10, 12), 3.25), biort, 1e-2)
    assert np.abs(z[:, :2] - 3.25).max() < 1e-14 and np.abs(z[:, 2:]).max() < 1e-14


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 3, 7, 9), (1, 2, 1, 5), (1, 1, 8, 6)])
def test_output_shape_also_for_odd_sizes(shape):
    b, c, h, w = shape
    x = np.random.default_rng(0).standard_normal(shape)
    z = R.scat_layer(x)
    assert z.shape == (b, 7 * c, -(-h // 2), -(-w // 2)) and np.isfinite(z).all()
    # an odd side is the even one with its last row / column repeated
    xe = np.concatenate((x, x[..., -1:, :]), axis=-2) if h % 2 else x
    xe = np.concatenate((xe, xe[..., :, -1:]), axis=-1) if w % 2 else xe
    assert np.array_equal(R.scat_layer(xe), z)
    assert R.scat_stack(x, 2).shape == (b, 49 * c, -(-(-(-h // 2)) // 2), -(-(-(-w // 2)) // 2))


def test_band_major_layout():
    C = 3
    for c in range(C):
        x = np.zeros((1, C, 12, 12))
        x[0, c] = np.random.default_rng(c).standard_normal((12, 12))
        z = R.scat_layer(x, magbias=1e-2)
        lit = sorted(k for k in range(7 * C) if np.abs(z[0, k]).max() > 1e-9)
        assert lit == [band * C + c for band in range(7)]


def test_orientation_selectivity():
    """A grating at 15, 45, ... 165 degrees peaks in magnitude band 1, 2, ... 6, well above its mirror image (the short level-1 filters are
    less one-sided in frequency than the q-shift ones test_dtcwt_cpu.py looks at: below a half, where those stay below 0.3)."""
    yy, xx = np.mgrid[0:64, 0:64].astype(float)
    for o, ang in enumerate(R.ANGLES):
        a = np.deg2rad(ang)
        img = np.cos(2 * np.pi * 0.36 * (np.sin(a) * xx + np.cos(a) * yy))
        z = R.scat_layer(img[None, None], magbias=0.0)
        e = np.array([(z[0, 1 + k] ** 2).sum() for k in range(6)])
        assert int(np.argmax(e)) == o, (ang, e)
        assert e[5 - o] < 0.5 * e[o], (ang, e)


def test_zero_magbias_is_the_plain_modulus_and_the_bias_only_smooths():
    from oracle import dtcwt_oracle as O

    x = np.random.default_rng(3).standard_normal((1, 2, 8, 10))
    _yl, yh = O.forward(x, 1)
    mod = np.sqrt((yh[0] ** 2).sum(-1))  # [B, C, 6, h, w]
    z = R.scat_layer(x, magbias=0.0)
    assert np.abs(z[:, 2:].reshape(1, 6, 2, 4, 5) - np.moveaxis(mod, 2, 1)).max() < 1e-15
    zb = R.scat_layer(x, magbias=0.5)
    assert (zb[:, 2:] <= z[:, 2:] + 1e-15).all() and (zb[:, 2:] >= 0).all() and np.array_equal(zb[:, :2], z[:, :2])


def test_the_tolerance_formula():
    # near_sym_a: ||h0o||_1 = 24 / 20, ||h1o||_1 = 352 / 280; (5 + 7 + 6) terms
    assert R.tolerance("near_sym_a", 2.0) == pytest.approx(18 * 2.0**-24 * (352 / 280) ** 2 * 2.0, rel=1e-12)
    assert R.tolerance("legall", 1.0) == pytest.approx(14 * 2.0**-24 * (12 / 8) ** 2, rel=1e-12)


# ---- window arithmetic ---------------------------------------------------------------------------------------------------------------
def _index_tensor(shape5):
    """A scattered tensor whose dim-2 slices are constant planes holding their own index."""
    z = np.zeros(shape5)
    z += np.arange(shape5[2]).reshape((1, 1, -1) + (1,) * (len(shape5) - 3))
    return z


@pytest.mark.parametrize("offset,first", [(0, 0), (-1, 24), (0.5, 12), (-0.25, 16)])
def test_channels_adjusted_window_literals(ng, offset, first):
    """C = 4, order 1: 28 channels, room (28 - 4) / 4 = 6 steps of 4.  -1 -> 6 + 1 - 1 = 6 -> 24; 0.5 -> round(3.0) = 3 -> 12;
    -0.25 -> 0.75 * 6 = 4.5 -> round half to even = 4 -> 16."""
    assert ng.scatternet_window(out_size=28, initial_size=4, increment=4, output_offset=offset) == first
    z = _index_tensor((1, 2, 28, 8, 8))
    got = R.window(z, shape=(2, 4, 8, 8), output_mode="channels_adjusted", output_offset=offset)
    assert got.shape == (2, 4, 8, 8) and [got[0, c, 0, 0] for c in range(4)] == [first + c for c in range(4)]


def test_flat_adjusted_window_literals(ng):
    """8 x 8 latent, C = 4: the inner plane is 16 x 16, the scattered tensor [1, B, 28, 8, 8] = 1792 elements per sample, of which 256 are
    kept: room 1536.  0.5 -> round(768.0) = 768 (channel 12, element 0); 3 -> element 3: a window that starts mid-row and ends in channel 4."""
    assert ng.scatternet_window(out_size=1792, initial_size=256, increment=1, output_offset=0.5) == 768
    assert ng.scatternet_window(out_size=1792, initial_size=256, increment=1, output_offset=3) == 3
    assert ng.scatternet_window(out_size=1792, initial_size=256, increment=1, output_offset=-1) == 1536
    z = np.arange(2 * 1792, dtype=np.float64).reshape(1, 2, 28, 8, 8)
    got = R.window(z, shape=(2, 4, 8, 8), output_mode="flat_adjusted", output_offset=0.5)
    assert np.array_equal(got.reshape(2, -1), np.stack([np.arange(768, 1024), 1792 + np.arange(768, 1024)]))
    got = R.window(z, shape=(2, 4, 8, 8), output_mode="flat_adjusted", output_offset=3)
    assert np.array_equal(got.reshape(2, -1)[0], np.arange(3, 259))


def test_plain_channels_window_crop_and_raw_reshape(ng):
    """`channels`, order 1, C = 4 on an 8 x 8 latent with an 8 x 8 inner plane: 4 C = 16 channels of 4 x 4, the crop to 8 x 8 changes
    nothing, and the 16 small planes are raw-reshaped into 4 channels of 8 x 8."""
    assert ng.scatternet_window(out_size=28, initial_size=16, increment=4, output_offset=-1) == 12
    z = _index_tensor((1, 1, 28, 4, 4))
    got = R.window(z, shape=(1, 4, 8, 8), output_mode="channels", output_offset=-1)
    assert np.array_equal(got.reshape(16, 16)[:, 0], np.arange(12, 28)) and got.shape == (1, 4, 8, 8)
    # an enlarged inner plane leaves planes larger than the latent: cropped, and then too many values for the reshape
    with pytest.raises(ValueError):
        R.window(_index_tensor((1, 1, 28, 16, 16)), shape=(1, 4, 8, 8), output_mode="channels", output_offset=0)


def test_per_channel_window_in_both_layouts():
    # channels_adjusted: [C, B, 7, h, w], one band kept per channel, squeeze + movedim -> [B, C, h, w]
    z = _index_tensor((4, 2, 7, 8, 8)) + 10 * np.arange(4).reshape(4, 1, 1, 1, 1) + 100 * np.arange(2).reshape(1, 2, 1, 1, 1)
    got = R.window(z, shape=(2, 4, 8, 8), output_mode="channels_adjusted", output_offset=-1, per_channel=True)
    assert np.array_equal(got[:, :, 0, 0], np.array([[6, 16, 26, 36], [106, 116, 126, 136]]))
    # flat_adjusted: per channel 7 * 64 elements, 64 kept
    z = np.arange(4 * 2 * 448, dtype=np.float64).reshape(4, 2, 7, 8, 8)
    got = R.window(z, shape=(2, 4, 8, 8), output_mode="flat_adjusted", output_offset=0.5, per_channel=True)
    assert np.array_equal(got[1, 2].ravel(), z[2, 1].ravel()[192:256])
    # plain channels, order 1: four bands per channel stay a dimension through movedim ([B, C, 4, h, w]) and are raw-reshaped
    z = _index_tensor((4, 1, 7, 4, 4)) + 10 * np.arange(4).reshape(4, 1, 1, 1, 1)
    got = R.window(z, shape=(1, 4, 8, 8), output_mode="channels", output_offset=1, per_channel=True)
    assert np.array_equal(got.reshape(4, 4, 16)[:, :, 0], np.array([[1, 2, 3, 4], [11, 12, 13, 14], [21, 22, 23, 24], [31, 32, 33, 34]]))


def _gen(ng, monkeypatch, shape=(2, 4, 8, 8), **kw):
    """A generator on a CPU latent with the device check of NoiseGenerator.update_x taken out: only its host arithmetic is used."""
    monkeypatch.setattr(ng.NoiseGenerator, "update_x", lambda self, x: (setattr(self, "shape", x.shape), setattr(self, "batch", x.shape[0]),
                        setattr(self, "channels", x.shape[1]), setattr(self, "height", x.shape[2]), setattr(self, "width", x.shape[3]),
                        setattr(self, "frames", None)) and None)
    return ng.ScatternetFilteredNoiseGenerator(torch.zeros(shape), **kw)


def test_the_generators_plan_is_the_window_before_the_last_layer(ng, monkeypatch):
    g = _gen(ng, monkeypatch, output_offset=-0.25)
    p = g.plan((2, 4, 16, 16))
    assert (p["k0"], p["nk"], p["h"], p["w"], p["output_mode"]) == (16, 4, 8, 8, "channels")
    p = _gen(ng, monkeypatch, output_mode="flat_adjusted", output_offset=3).plan((2, 4, 16, 16))
    assert (p["k0"], p["nk"], p["lo"], p["initial_size"]) == (0, 5, 3, 256)  # elements 3 .. 258: channels 0 .. 4
    p = _gen(ng, monkeypatch, output_mode="flat_adjusted", output_offset=0.5).plan((2, 4, 16, 16))
    assert (p["k0"], p["nk"], p["lo"]) == (12, 4, 0)
    p = _gen(ng, monkeypatch, output_mode="channels", output_offset=-1).plan((2, 4, 8, 8))
    assert (p["k0"], p["nk"]) == (12, 16)
    p = _gen(ng, monkeypatch, output_mode="channels_scaled", scatternet_order=-2, output_offset=-1).plan((2, 4, 32, 32))
    assert (p["k0"], p["nk"], p["h"], p["order"]) == (192, 4, 8, 2)
    p = _gen(ng, monkeypatch, scatternet_order=3, per_channel_scatternet=True, output_offset=-1).plan((2, 4, 64, 64))
    assert (p["k0"], p["nk"], p["h"]) == (342, 1, 8)
    # a window past the end, and one that cannot fill the latent: before any launch
    with pytest.raises(ValueError, match="runs outside the scattered output"):
        _gen(ng, monkeypatch, output_offset=7).plan((2, 4, 16, 16))
    with pytest.raises(ValueError, match="the latent .* needs"):
        _gen(ng, monkeypatch).plan((2, 4, 8, 8))
    with pytest.raises(ValueError, match="the latent .* needs"):
        _gen(ng, monkeypatch, output_mode="channels").plan((2, 4, 16, 16))


# ---- refusals, at construction, on the host --------------------------------------------------------------------------------------------
def test_refusals_at_construction(ng, nz):
    G = ng.ScatternetFilteredNoiseGenerator
    assert G.name == "scatternetfilter" and G.MIN_DIMS == G.MAX_DIMS == 4 and issubclass(G, ng.FramesToChannelsNoiseGenerator)
    want = {"mode": "symmetric", "magbias": 1e-02, "use_symmetric_filter": False, "biort": "near_sym_a", "qshift": "qshift_a",
            "output_offset": 0.0, "scatternet_order": 1, "per_channel_scatternet": False, "output_mode": "channels_adjusted",
            "upscale_mode": None, "noise_sampler": None}
    params = G.ng_params()
    assert {k: params[k] for k in want} == want
    x = torch.zeros(1, 4, 8, 8)  # a CPU latent: everything below is raised before the device check
    with pytest.raises(NotImplementedError, match=r"ScatLayerj2.*-2 is the stack of two first-order layers"):
        G(x, scatternet_order=2)
    with pytest.raises(NotImplementedError, match="symmetric extension only"):
        G(x, mode="zero")
    with pytest.raises(NotImplementedError, match="near_sym_b_bp.*absent pytorch_wavelets"):
        G(x, use_symmetric_filter=True)
    with pytest.raises(NotImplementedError, match="near_sym_b.*built in: near_sym_a, legall, antonini"):
        G(x, biort="near_sym_b")
    with pytest.raises(ValueError, match="Bad output mode"):
        G(x, output_mode="channels_flat")
    with pytest.raises(ValueError, match="requires at most 4 dimension"):
        G(torch.zeros(1, 4, 2, 8, 8))
    with pytest.raises(nz.hip_lib.SonarHipError, match="only runs on a ROCm device"):
        G(x)
    for order in (1, -1, -2, 3, -3, 0):
        with pytest.raises(nz.hip_lib.SonarHipError):  # these pass the refusals and reach the device check
            G(x, scatternet_order=order)
    # the item: the same refusals, and its own for a latent that is not 4-D
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    with pytest.raises(ValueError, match="Currently can only handle 4 dimensional latents"):
        nz.ScatternetFilteredNoise(1.0, noise=chain).make_noise_sampler(torch.zeros(1, 4, 2, 8, 8), 0.03, 14.6)
    with pytest.raises(NotImplementedError, match="ScatLayerj2"):
        nz.ScatternetFilteredNoise(1.0, noise=chain, scatternet_order=2).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True)
    with pytest.raises(NotImplementedError, match="symmetric extension only"):
        nz.ScatternetFilteredNoise(1.0, noise=chain, padding_mode="reflect").make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True)
    with pytest.raises(nz.hip_lib.SonarHipError):
        nz.ScatternetFilteredNoise(1.0, noise=None).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True)


def test_wrapper_refusals_without_a_device(pkg):
    hl = pkg.hip_lib
    with pytest.raises(hl.SonarHipError, match="ROCm device"):
        hl.scat_layer(torch.zeros(1, 2, 8, 8))
    with pytest.raises(hl.SonarHipError, match="channel window"):
        hl.scat_layer(torch.zeros(1, 2, 8, 8), channels=(13, 2))
    with pytest.raises(hl.SonarHipError, match="channel window"):
        hl.scat_layer(torch.zeros(1, 2, 8, 8), channels=(0, 0))
    with pytest.raises(hl.SonarHipError, match=r"\[B, C, H, W\]"):
        hl.scat_layer(torch.zeros(2, 8, 8))
    with pytest.raises(NotImplementedError, match="built in"):
        hl.scat_layer(torch.zeros(1, 2, 8, 8), biort="near_sym_b")
    assert list(inspect.signature(hl.scat_layer).parameters) == ["x", "biort", "magbias", "channels", "out"]


def test_entry_point_is_declared_bound_and_exported(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64}
    name = "sonar_scat_layer_f32"
    decl = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", text)
    assert decl is not None
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = hl.SIGNATURES[name]
    assert restype is hl.C.c_int and len(params) == len(argtypes) == 14
    for p, a in zip(params, argtypes):
        typ = p.rsplit(" ", 1)[0]
        assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), p
    assert hasattr(hl.load(), name)
    define = lambda n: int(re.search(rf"#define {n} (\d+)", text).group(1))  # noqa: E731
    assert (define("SONAR_SCAT_TILE_H"), define("SONAR_SCAT_TILE_W")) == (hl.SCAT_TILE_H, hl.SCAT_TILE_W)
    assert os.path.exists(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "scatternet.hip"))


def test_bad_arguments_come_back_as_error_codes_without_a_device(pkg):
    """Everything is checked before the launch: the device pointers below are never dereferenced."""
    hl = pkg.hip_lib
    lib = hl.load()
    F = hl.C.c_float
    h5, h7, h3, h9 = (F * 5)(*[0.2] * 5), (F * 7)(*[0.1] * 7), (F * 3)(*[0.3] * 3), (F * 9)(*[0.1] * 9)
    ok = dict(x=0x1000, out=0x200000, B=1, C=2, H=8, W=8, h0=h5, n0=5, h1=h7, n1=7, bias=1e-2, k0=0, nk=14)

    def call(**kw):
        a = ok | kw
        return lib.sonar_scat_layer_f32(a["x"], a["out"], a["B"], a["C"], a["H"], a["W"], a["h0"], a["n0"], a["h1"], a["n1"], a["bias"], a["k0"],
                                        a["nk"], None)

    for bad in (dict(x=None), dict(out=None), dict(h0=None), dict(h1=None), dict(out=0x1000), dict(x=0x1002), dict(out=0x200001), dict(B=-1),
                dict(C=0), dict(H=0), dict(W=0), dict(bias=-1.0), dict(bias=float("nan")), dict(bias=float("inf")), dict(k0=-1), dict(nk=0),
                dict(k0=13, nk=2), dict(k0=14, nk=1), dict(h0=(F * 5)(0.1, float("nan"), 0.1, 0.1, 0.1))):
        assert call(**bad) == hl.ERR_ARG, bad
    assert call(k0=13, nk=2) == hl.ERR_ARG and b"channel window" in lib.sonar_last_error()
    for bad in (dict(n0=7, h0=h7, n1=5, h1=h5), dict(n0=9, h0=h9, n1=3, h1=h3), dict(n0=5, n1=5, h1=h5), dict(H=2**20 + 1), dict(W=2**21)):
        assert call(**bad) == hl.ERR_UNSUPPORTED, bad
    assert call(n0=5, n1=5, h1=h5) == hl.ERR_UNSUPPORTED and b"5 / 7, 5 / 3, 9 / 7" in lib.sonar_last_error()
    assert call(B=0) == 0  # nothing to do, nothing launched


# ---- the item ------------------------------------------------------------------------------------------------------------------------------
class _Inner:
    """A chain stand-in whose sampler is one known object; remembers how it was asked."""

    def __init__(self):
        self.sampler = lambda s, sn: None
        self.asked = []

    def clone(self):
        return self

    def make_noise_sampler(self, x, *a, **k):
        self.asked.append((tuple(x.shape), x.dtype, k))
        return self.sampler


def test_the_item_signature_clone_and_inner_request(nz):
    assert issubclass(nz.ScatternetFilteredNoise, nz.CustomNoiseItemBase)
    params = inspect.signature(nz.ScatternetFilteredNoise.__init__).parameters
    assert list(params) == ["self", "factor", "noise", "padding_mode", "use_symmetric_filter", "magbias", "output_offset", "output_mode",
                            "scatternet_order", "per_channel_scatternet", "normalize_noise", "normalize", "kwargs"]
    assert [params[k].default for k in list(params)[2:-1]] == [None, "symmetric", False, 1e-2, 0.0, "channels_adjusted", 1, False, False, None]
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.ScatternetFilteredNoise(0.7, noise=chain, output_offset=-1, scatternet_order=-2, normalize_noise=True, normalize=False)
    clone = item.clone()
    assert clone.noise is not item.noise and clone.keys == item.keys and "noise" in clone.keys
    assert (clone.factor, clone.output_offset, clone.scatternet_order, clone.normalize_noise, clone.normalize) == (0.7, -1, -2, True, False)
    assert item.clone_key("noise") is not item.noise and item.clone_key("magbias") == 1e-2
    none = nz.ScatternetFilteredNoise(1.0)
    assert none.clone_key("noise") is None and none.clone().noise is None
    # the inner chain is asked for the plane enlarged by 2**|order| in the _adjusted modes only, with normalized=normalize_noise; the
    # generator then refuses the CPU latent (no host fallback)
    x = torch.zeros(2, 4, 8, 6)
    for mode, order, normalize_noise, want in (("channels_adjusted", 1, False, (2, 4, 16, 12)), ("flat_adjusted", -2, True, (2, 4, 32, 24)),
                                               ("channels_adjusted", 3, True, (2, 4, 64, 48)), ("channels_adjusted", 0, False, (2, 4, 8, 6)),
                                               ("channels", 1, False, (2, 4, 8, 6)), ("flat", 3, True, (2, 4, 8, 6)),
                                               ("channels_scaled", 1, True, (2, 4, 8, 6)), ("flat_scaled", -2, False, (2, 4, 8, 6))):
        inner = _Inner()
        it = nz.ScatternetFilteredNoise(1.0, noise=inner, output_mode=mode, scatternet_order=order, normalize_noise=normalize_noise)
        with pytest.raises(nz.hip_lib.SonarHipError):
            it.make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True, normalized=True)
        shape, dtype, k = inner.asked[-1]
        assert shape == want and dtype == torch.float32 and k["normalized"] is normalize_noise, (mode, order)
        assert k["sigma_min"] == 0.03 and k["sigma_max"] == 14.6 and k["seed"] == 1 and k["cpu"] is True
    # a half latent: the chain is built for its fp32 image
    inner = _Inner()
    with pytest.raises(nz.hip_lib.SonarHipError):
        nz.ScatternetFilteredNoise(1.0, noise=inner).make_noise_sampler(x.to(torch.bfloat16), 0.03, 14.6, seed=1, cpu=True)
    assert inner.asked[-1][:2] == ((2, 4, 16, 12), torch.float32)
    # a refusal comes before the chain is asked at all
    inner = _Inner()
    with pytest.raises(NotImplementedError):
        nz.ScatternetFilteredNoise(1.0, noise=inner, scatternet_order=2).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True)
    assert inner.asked == []


def test_the_registry_is_unchanged(reg, ng):
    assert len(reg.NODE_CLASS_MAPPINGS) == 54 and len(reg.IMPLEMENTED_KEYS) == 42
    off = sorted(k for k, cls in reg.NODE_CLASS_MAPPINGS.items() if cls.__name__.startswith("OffPath_"))
    assert len(off) == 12 and not set(off) & set(reg.IMPLEMENTED_KEYS)
    assert "SonarScatternetFilteredNoise" in off and "SonarScatternetFilteredNoise" not in reg.IMPLEMENTED_KEYS
    assert len(ng.NoiseType) == 38
