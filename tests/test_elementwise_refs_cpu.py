"""CPU: the references of tests/elementwise_refs.py themselves, so that tests/test_gpu_elementwise.py cannot pass or fail for the
reference's reasons.  Each restatement that has a float32 sibling in oracle/sonar_oracle.py or a committed golden is run in float64 on
the sibling's inputs and agrees with it at the project's elementwise tolerance; the two DPM++ half steps, chained, reproduce the committed
traces; the input generators produce what their tests claim."""
import pytest
import torch

from oracle import sonar_oracle as orc
from tests import elementwise_refs as R
from tests.test_gpu_host_api import MOMENTUM_CASES
from tests.test_gpu_kernels import CFGS, close
from tests.test_oracle_golden import fake_model, to_cfg


def seeded(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ momentum
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: f"{c.mode}-{c.init}-{c.blend_mode}-m{c.momentum}-h{c.momentum_hist}")
def test_euler_reference_follows_the_oracle_step(cfg):
    """Three chained steps: R.euler_step in float64 (history handed over explicitly) == MomentumState.euler_step in float32."""
    x = seeded(2, 4, 8, 8, seed=9)
    st = orc.MomentumState(cfg)
    sig = [7.0, 4.0, 2.0, 1.0]
    h64 = None
    for step in range(3):
        den = x * 0.5 + torch.tanh(x) * 0.1
        want = st.euler_step(step, x, den, torch.tensor(sig[step]), torch.tensor(sig[step + 1]))
        got, h64 = R.euler_step(cfg, step, x.double(), den.double(), h64, sig[step], sig[step + 1] - sig[step])
        close(got.float(), want)
        assert (h64 is None) == (st.h is None)
        if h64 is not None:
            close(h64.float(), st.h)
            h64 = st.h.double()
        x = want


@pytest.mark.parametrize("mode", ["NEW", "DENOISED"])
def test_rand_init_reference_hands_the_fresh_history_in(mode):
    cfg = orc.MomentumCfg(init="RAND", mode=mode)
    x, den, h0 = seeded(1, 4, 8, 8, seed=1), seeded(1, 4, 8, 8, seed=2), seeded(1, 4, 8, 8, seed=3)
    st = orc.MomentumState(cfg, rand_init=lambda: h0.clone())
    want = st.euler_step(0, x, den, torch.tensor(3.0), torch.tensor(2.0))
    got, h = R.euler_step(cfg, 0, x.double(), den.double(), h0.double(), 3.0, -1.0, h_fresh=True)
    close(got.float(), want)
    close(h.float(), st.h)
    # the same history, not fresh: DENOISED mode mixes it into the denoised prediction before the update (the other modes never do)
    stale, _ = R.euler_step(cfg, 0, x.double(), den.double(), h0.double(), 3.0, -1.0)
    assert torch.allclose(stale, got) == (mode != "DENOISED")


@pytest.mark.parametrize("name", list(MOMENTUM_CASES))
def test_dpmpp_half_step_references_reproduce_the_committed_traces(golden, name):
    """R.dpmpp_stage1 -> model -> R.dpmpp_stage2 per step (the last step, to sigma 0, is R.euler_step), in float64 with the golden's model
    and noise bank, against the dpmpp_* traces of momentum.npz at test_momentum_traces' tolerance."""
    g = golden("momentum")
    cfg = to_cfg(MOMENTUM_CASES[name])
    bank = iter(g["noise_bank"])
    x, h = g["x0"].double(), None
    sigmas = g["sigmas"].double()
    want = g[f"dpmpp_{name}"]
    assert want.shape[0] == len(sigmas) - 1
    for i in range(len(sigmas) - 1):
        sigma, sigma_next = sigmas[i], sigmas[i + 1]
        s_in = x.new_ones((x.shape[0],))
        den = fake_model(x, sigma * s_in)
        if sigma_next == 0:
            down, _ = orc.ancestral_step(sigma, sigma_next, 0.9)
            x, h = R.euler_step(cfg, i, x, den, h, sigma, down - sigma)
        else:
            adj = cfg.momentum + (1 - cfg.momentum) / 2 if h is not None else cfg.momentum
            k = R.dpmpp_scalars(sigma, sigma_next, 0.9, 1.05)
            x2, md1, h = R.dpmpp_stage1(cfg, i, x, den, h, k["sigma"], k["expm1_a"], k["ratio_a"], adj == 1, noise=next(bank).double(),
                                        noise_scale=k["noise_scale_a"])
            den2 = fake_model(x2, k["sigma_s"] * s_in)
            x, _dd, h = R.dpmpp_stage2(cfg, i, x, den2, md1, h, k["sigma_s"], k["expm1_b"], k["ratio_b"], k["fac"], adj == 1,
                                       noise=next(bank).double(), noise_scale=k["noise_scale_b"])
        close(x.float(), want[i], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("case", list(R.NORM_OUTCOMES))
@pytest.mark.parametrize("shape", [(4, 4, 64, 64), (2, 4, 8, 8), (1, 3, 7, 5)])
def test_norm_reference_takes_the_decision_of_scale_noise(case, shape):
    """R.norm_decision / R.apply_norm == oracle.scale_noise(normalized=True), and the generator's three cases give the three outcomes
    at every shape the GPU tests use them at, with a margin (no decision sits near its threshold)."""
    noise, factor = R.norm_noise(case, shape)
    dec = {}
    want = orc.scale_noise(noise.clone(), factor, normalized=True, decisions=dec)
    mean, sd, sub, div, _f = d = R.norm_decision(noise.double(), factor)
    assert (sub, div) == (dec["sub"], dec["div"]) == R.NORM_OUTCOMES[case]
    thr = dec["threshold"]
    for value, taken in ((abs(mean), sub), (abs(1.0 - sd), div)):
        assert value > 1.5 * thr if taken else value < 0.5 * thr, (value, thr)
    close(R.apply_norm(noise.double(), d).float(), want)


# ------------------------------------------------------------------------------------------------ noise-type helpers with a sibling
@pytest.mark.parametrize("alpha,use_sign", [(0.0, True), (0.5, True), (1.0, False), (1.5, False), (0.7, True), (2.0, False), (2.5, True)])
def test_powerlaw_reference(golden, alpha, use_sign):
    draw = golden("powerlaw")["draw"]
    close(R.powerlaw(draw.double(), alpha, use_sign).float(), orc.powerlaw_noise(draw, alpha=alpha, use_sign=use_sign))
    assert torch.equal(R.powerlaw(draw, alpha, use_sign), orc.powerlaw_noise(draw, alpha=alpha, use_sign=use_sign))


def test_powerlaw_reference_against_the_golden(golden):
    g = golden("powerlaw")
    close(R.powerlaw(g["draw"].double(), 1.0, False).float(), g["adv_a1_none"])
    close(R.powerlaw(g["draw"].double(), 0.0, True).float(), g["white_0"])


def test_laplace_reference(golden):
    g = golden("basic_types")
    torch.manual_seed(22)
    n = torch.randn(3, 4, 8, 8)
    u = torch.empty(3, 4, 8, 8).uniform_(torch.finfo(torch.float32).eps - 1, 1)
    got = R.laplace_add(n.double(), u.double(), 4.0, 0.0, 1.0).float()
    close(got, orc.laplacian_noise(n, u))
    close(got, g["laplacian_0"])
    # sign(0) = 0 and the clamp at tiny: u = 0 adds exactly loc
    assert torch.equal(R.laplace_add(torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), 4.0, 0.5, 2.0), torch.full((2,), 0.75, dtype=torch.float64))


def test_studentt_and_clamp_signpow_references(golden):
    """studentt + the quantile clamp + the signed power == oracle.studentt_noise == the golden."""
    g = golden("basic_types")
    xn, gm = g["studentt_normal_draw"], g["studentt_gamma_draw"]
    raw = R.studentt(xn.double(), gm.double(), 0.0, 0.2, 1.0)
    nq = torch.quantile(raw.float().flatten(start_dim=1).abs(), 0.75, dim=-1)
    got = R.clamp_signpow_rows(raw.flatten(start_dim=1), nq.double(), 1.0, 0.5).reshape(xn.shape).float()
    close(got, orc.studentt_noise(xn, gm))
    close(got, g["studentt_0"])


def test_normalize_to_scale_reference(golden):
    """In float32 the restatement IS the reference's op sequence: bit for bit on the committed vectors, the span rounded once included;
    in float64 it agrees at the elementwise tolerance."""
    g = golden("resample_modes")
    x = g["nts_in"]
    b = x.shape[0]
    for lo, hi, key in ((0.0, 1.0, "nts_default"), (0.1, 0.3, "nts_inexact")):
        assert torch.equal(R.normalize_to_scale(x.reshape(b, -1), lo, hi).reshape(x.shape), g[key])
        assert torch.equal(orc.normalize_to_scale(x, lo, hi), g[key])
        close(R.normalize_to_scale(x.double().reshape(b, -1), lo, hi).reshape(x.shape).float(), g[key])
    rows = x.shape[0] * x.shape[1]
    assert torch.equal(R.normalize_to_scale(x.reshape(rows, -1), -1.5, 2.0).reshape(x.shape), g["nts_hw"])
    assert torch.equal(R.normalize_to_scale(x.reshape(1, -1), 0.25, 0.5, eps=1e-3).reshape(x.shape), g["nts_all"])
    # the once-rounded span is visible in float32: 0.3f - 0.1f differs from float(0.3 - 0.1)
    wrong = (x.reshape(b, -1) - x.reshape(b, -1).amin(1, keepdim=True)) / ((x.reshape(b, -1).amax(1, keepdim=True) - x.reshape(b, -1).amin(1, keepdim=True)) + 1e-7)
    wrong = (wrong * (torch.tensor(0.3) - torch.tensor(0.1)) + 0.1).clamp(0.1, 0.3)
    assert not torch.equal(wrong.reshape(x.shape), g["nts_inexact"])


def test_signed_rescale_reference_against_the_reference_vectors():
    rows, names, cases = R.load_signed_rescale_golden()
    assert set(cases) >= {"fixed", "auto", "skip_neg", "skip_pos", "inexact"}
    for name, (targets, want) in cases.items():
        got32 = R.signed_rescale(rows, *targets)
        assert torch.equal(got32, want), name  # the reference's own op sequence
        close(R.signed_rescale(rows.double(), *targets).float(), want)
    # the skipped sign is copied, the other one is not
    neg = rows < 0
    assert torch.equal(cases["skip_neg"][1][neg], rows[neg]) and not torch.equal(cases["skip_neg"][1][rows > 0], rows[rows > 0])
    assert torch.equal(cases["skip_pos"][1][rows > 0], rows[rows > 0])


def test_signed_rescale_fixture_rows_are_what_their_names_say():
    rows, names, cases = R.load_signed_rescale_golden()
    row = dict(zip(names, rows))
    assert bool((row["mixed"] < 0).any()) and bool((row["mixed"] > 0).any()) and not bool((row["mixed"] == 0).any())
    assert bool((row["all_positive"] > 0).all())
    assert not bool((row["all_negative"] >= 0).any())
    z = row["with_zeros"]
    assert int((z == 0).sum()) == 4 and bool(torch.signbit(z[4])) and bool((z < 0).any()) and bool((z > 0).any())
    assert int((row["one_each"] > 0).sum()) == 1 and int((row["one_each"] < 0).sum()) == 1
    assert not bool(row["all_zero"].any())
    mn, mx, mp, xp = cases["auto"][0]
    assert mx >= 0 and mp < 0  # both data-derived targets
    assert cases["auto_neg_only"][0][1] >= 0 and cases["auto_neg_only"][0][2] >= 0
    assert cases["auto_pos_only"][0][1] < 0 and cases["auto_pos_only"][0][2] < 0
    assert cases["skip_neg"][0][0] >= 0 and cases["skip_pos"][0][3] <= 0
    # a data-derived target: the largest negative of the row maps onto itself, the smallest positive too
    out = cases["auto"][1][names.index("mixed")]
    m = row["mixed"]
    close(out[m < 0].max(), m[m < 0].max())
    close(out[m > 0].min(), m[m > 0].min())


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_bcast_gain_reference_is_the_modulation_gain(dims):
    """bcast mode 2 / 1 / 0 == std over dim -3 / (-2, -1) / (-3, -2, -1) (oracle.MODULATION_DIMS), v = plain * gain + plain."""
    ref, noise = seeded(2, 3, 5, 7, seed=4, scale=1.3), seeded(2, 3, 5, 7, seed=5)
    b, c, h, w = ref.shape
    want = noise * orc._modulation_gain(ref, -0.6, orc.MODULATION_DIMS[dims - 1]) + noise
    bcast = {1: 2, 2: 1, 3: 0}[dims]
    centred = (ref - ref.mean()).double()
    sd = {2: R.std_mid(centred.reshape(b, c, h * w)), 1: centred.reshape(b * c, h * w).std(dim=1), 0: centred.reshape(b, -1).std(dim=1)}[bcast]
    got, sx, sv = R.bcast_gain(noise.double().reshape(b, c, h * w), sd, bcast, 0.6, 1.0)
    close(got.reshape(ref.shape).float(), want)
    assert abs(float(sx) - float((noise.double() ** 2).sum())) < 1e-9 and abs(float(sv) - float((got * got).sum())) < 1e-9
    n64 = noise.double().reshape(b, c, h * w)
    shaped = got * (torch.norm(n64) / torch.norm(got))
    close(R.ratio_mix(got, -0.6, n64, 1.6, sx, 1.0, sv).float(), (shaped * -0.6 + n64 * 1.6).float())


# ------------------------------------------------------------------------------------------------ the rest: identities
def test_std_and_amax_references():
    x = seeded(3, 4, 35, seed=6) + 1000.0
    two_pass = ((x.double() - x.double().mean(1, keepdim=True)) ** 2).sum(1).div(3).sqrt()
    close(R.std_mid(x.double()).float(), two_pass.float())
    naive = ((x * x).sum(1) - x.sum(1) ** 2 / 4).div(3).clamp(min=0).sqrt()  # float32 sum of squares at 1000 + N(0, 1): useless
    assert float((naive.double() - two_pass).abs().max()) > 1e-2
    assert bool(torch.isnan(R.std_mid(torch.ones(2, 1, 8, dtype=torch.float64))).all())
    y = -seeded(2, 3, 5, seed=7).abs() - 1.0
    assert bool((R.amax_mid(y, False) < 0).all()) and bool((R.amax_mid(y, True) > 0).all())
    y[1, 2, 3] = float("nan")
    nan = torch.isnan(R.amax_mid(y, False))
    assert int(nan.sum()) == 1 and bool(nan[1, 3])


def test_spectral_references():
    x = seeded(2, 3, 5, 7, seed=8).double()
    z = torch.fft.fft(x.reshape(2, 3, 35), dim=1)
    back = R.cdft_mid(R.cdft_mid(x.reshape(2, 3, 35), False, False), True, True) / 3
    close(back.float(), x.reshape(2, 3, 35).float())
    assert torch.equal(R.cdft_mid(x.reshape(2, 3, 35), False, False), z)
    for channel_dft in (False, True):
        full = R.full_abs_logamp(x, channel_dft)
        spec = R.spectrum_of(x, channel_dft)
        half = spec[..., :4]
        assert torch.allclose(R.logamp(half).abs(), full[..., :4])
        # the dropped columns are the Hermitian partners' (channel flipped too under a channel DFT)
        for kx in (4, 5, 6):
            for ky in range(5):
                for c in range(3):
                    src = half[:, (3 - c) % 3 if channel_dft else c, (5 - ky) % 5, 7 - kx]
                    assert torch.allclose(R.logamp(src).abs(), full[:, c, ky, kx], atol=1e-12)
    # signum mask: every branch of the multiplier
    q = (torch.tensor(2.0), torch.tensor(4.0), torch.tensor(6.0))
    a = torch.tensor([0.5, 1.5, 3.0, 4.5, 5.5, 7.0], dtype=torch.float64)
    want = torch.tensor([1.5, 1.25, 1.0, 0.75, 0.5, 0.5], dtype=torch.float64)
    assert torch.allclose(R.signum_mult(a, q, 1.0), want) and torch.allclose(R.signum_mult(a, q, 2.0), want**2)


def test_helper_references_small_identities():
    x = torch.tensor([[1.0, -2.0, 0.0, -0.0, 3.0, -0.5]], dtype=torch.float64)
    out = R.clamp_signpow_rows(x, torch.tensor([2.0], dtype=torch.float64), 0.5, 2.0)
    assert torch.equal(out, torch.tensor([[1.0, -1.0, 0.0, -0.0, 1.0, -0.25]], dtype=torch.float64)) and bool(torch.signbit(out[0, 3]))
    t = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    v = R.mul_table(torch.ones(12, dtype=torch.float64), t, 2, True)
    assert torch.equal(v, torch.tensor([0.5, 0.5, 1.0, 1.0, -2.0, -2.0] * 2, dtype=torch.float64)) and not bool(torch.signbit(v[2]))
    assert torch.equal(R.mul_table(-torch.ones(4, dtype=torch.float64), t[1:2], 1, True), torch.ones(4, dtype=torch.float64))  # 1 - s = +0
    assert torch.equal(R.sq_acc(torch.full((3,), 9.0), torch.tensor([1.0, 2.0, 3.0]), 0.5, True), torch.tensor([0.5, 2.0, 4.5]))
    assert R.ref32_error(R.powerlaw, seeded(64, seed=1).double(), 2.0, False) < 1e-6
    assert 0 < R.ref32_error(R.powerlaw, seeded(64, seed=1).double(), 1.7, False) < 1e-5
