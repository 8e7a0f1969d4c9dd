"""Kernel-level parity (-m gpu) of the sampler-step kernels (csrc/sampler_steps.hip) and of the helper entry points the noise types are
built from (csrc/elementwise.hip, csrc/rows.hip, csrc/spectral_ops.hip): every case is called through hip_lib and compared with a
float64 reference (tests/elementwise_refs.py, itself pinned by tests/test_elementwise_refs_cpu.py) of the float32 inputs the kernel
received, rounded once.

Tolerances
  exact (torch.equal)   : where a kernel only selects or copies -- amax_mid, NaN / zero placement, the skipped sign of signed_rescale,
                          which outputs exist, x_out with and without dd.
  project (R.within)    : everything built from + - x / sqrt: rtol 1e-5, atol 1e-6 at every element (tests/test_gpu_kernels.py).
  transcendental        : powf, log1pf, logf, sincospif sums: four times the error of the SAME restatement run in float32 on the host on the
                          test's own input (R.ref32_error), never less than the project tolerance.  The bound comes from the reference
                          alone; the values measured are written next to each test.
No element is dropped or masked except where the reference itself is NaN (positions placed in advance, compared in kind, below 1 % of
the test's elements: R.within asserts all three).

Left out: grid_stream's cap at 2^20 blocks (csrc/ew_driver.h) takes 2^30 elements to reach -- four 4 GiB operands for a step kernel.
"""
import pytest
import torch

from oracle import sonar_oracle as orc
from tests import elementwise_refs as R
from tests.test_gpu_kernels import CFGS, make_cfg

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 5, 1023, 4 * 1024 + 1]  # scalar-only, tail-only, one vector, vector + tail, odd, more than one block + tail


@pytest.fixture(scope="module")
def hl(pkg):
    lib = pkg.hip_lib
    lib.load()
    return lib


def seeded(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def put(t, off=0):
    """Device copy of t that starts `off` floats past a 16-byte boundary: buf[off : off + n] of a larger buffer."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v.view(t.shape)


def d64(*ts):
    return [None if t is None else t.double() for t in ts]


def nan_partials(hl):
    return torch.full((hl.NPART * 2,), float("nan"), dtype=torch.float64, device="cuda")


def same_values(a, b):
    """torch.equal that lets NaN equal NaN."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


# ================================================================================================ launch_ew family: layouts
def _norm_for_layout(hl):
    base, factor = R.norm_noise("shift_and_scale", (4096,), seed=5)
    norm = hl.norm_decision(hl.stats(base.cuda()), base.numel(), factor)
    return norm, R.norm_decision(base.double(), factor)


def _default_step_cfg(hl):
    c = orc.MomentumCfg()
    return c, make_cfg(hl, c, orc.MomentumState(c), 1, True)


SIG, DT, NSCALE = 3.0, -0.5, R.f32(0.77)
E1A, R1A, E1B, R1B, FAC = R.f32(-0.3), R.f32(0.8), R.f32(-0.4), R.f32(0.6), 0.75

# name -> (number of operands, run(hl, device operands) -> outputs, ref(float64 operands) -> outputs, transcendental?)
# an operand that is only written (an `out`) starts as a draw like the others; ref ignores it
LAYOUT_OPS = {
    "mul_scalar": (2, lambda hl, o: (hl.mul_scalar(o[0], 1.7, out=o[1]),), lambda o: (R.scalar_op(0, o[0], None, R.f32(1.7)),), False),
    "div_scalar": (2, lambda hl, o: (hl.div_scalar(o[0], 1.7, out=o[1]),), lambda o: (R.scalar_op(1, o[0], None, R.f32(1.7)),), False),
    "to_d": (3, lambda hl, o: (hl.to_d(o[0], o[1], 1.7, out=o[2]),), lambda o: (R.scalar_op(2, o[0], o[1], R.f32(1.7)),), False),
    "affine_": (1, lambda hl, o: (hl.affine_(o[0], 0.5, 3.46, 0.1),), lambda o: (R.affine(o[0], 0.5, R.f32(3.46), R.f32(0.1)),), False),
    "sq_acc_first": (2, lambda hl, o: (hl.sq_acc_(o[0], o[1], 0.3, True),), lambda o: (R.sq_acc(o[0], o[1], R.f32(0.3), True),), False),
    "sq_acc_next": (2, lambda hl, o: (hl.sq_acc_(o[0], o[1], 0.3, False),), lambda o: (R.sq_acc(o[0], o[1], R.f32(0.3), False),), False),
    "powerlaw_1.7": (1, lambda hl, o: (hl.powerlaw_(o[0], 1.7, False),), lambda o: (R.powerlaw(o[0], R.f32(1.7), False),), True),
    "powerlaw_sign_0.5": (1, lambda hl, o: (hl.powerlaw_(o[0], 0.5, True),), lambda o: (R.powerlaw(o[0], 0.5, True),), True),
    "laplace_add_": (2, lambda hl, o: (hl.laplace_add_(o[0], o[1], 4.0, 0.25, 1.5),), lambda o: (R.laplace_add(o[0], o[1], 4.0, 0.25, 1.5),), True),
    "studentt_": (2, lambda hl, o: (hl.studentt_(o[0], o[1], 0.1, 0.2, 3.0),), lambda o: (R.studentt(o[0], o[1], R.f32(0.1), R.f32(0.2), 3.0),), False),
    "euler": (6, lambda hl, o: hl.momentum_euler(o[0], o[1], o[2], _default_step_cfg(hl)[1], SIG, DT, noise=o[3], noise_scale=NSCALE, x_out=o[4], h_out=o[5]),
              lambda o: R.euler_step(orc.MomentumCfg(), 1, o[0], o[1], o[2], SIG, DT, noise=o[3], noise_scale=NSCALE), False),
    "dpmpp_stage1": (4, lambda hl, o: hl.dpmpp_stage1(o[0], o[1], o[2], _default_step_cfg(hl)[1], SIG, E1A, R1A, False, noise=o[3], noise_scale=NSCALE),
                     lambda o: R.dpmpp_stage1(orc.MomentumCfg(), 1, o[0], o[1], o[2], SIG, E1A, R1A, False, noise=o[3], noise_scale=NSCALE), False),
    "dpmpp_stage2": (5, lambda hl, o: hl.dpmpp_stage2(o[0], o[1], o[2], o[3], _default_step_cfg(hl)[1], SIG, E1B, R1B, FAC, False, noise=o[4], noise_scale=NSCALE,
                                                      want_dd=True),
                     lambda o: R.dpmpp_stage2(orc.MomentumCfg(), 1, o[0], o[1], o[2], o[3], SIG, E1B, R1B, FAC, False, noise=o[4], noise_scale=NSCALE), False),
}


def _layout_inputs(name, count, n):
    ops = [seeded(n, seed=100 + 7 * k + n % 97) for k in range(count)]
    if name == "laplace_add_":  # the uniform of Laplace.rsample, in (eps - 1, 1), with a zero and both ends
        u = torch.rand(n, generator=torch.Generator().manual_seed(n)) * 2 - 1
        u[0] = 0.0
        if n > 4:
            u[1], u[2] = float(torch.finfo(torch.float32).eps) - 1, 1 - 2.0**-24
        ops[1] = u
    if name == "studentt_":  # gamma draws: positive, one at zero (clamped to tiny)
        ops[1] = ops[1].abs() * 0.5 + 0.01
        ops[1][-1] = 0.0
    return ops


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(LAYOUT_OPS))
def test_launch_ew_family_sizes_and_alignment(hl, name, n):
    """Every operand contiguous and 16-byte aligned (the float4 kernel: vector body + the tail block 0 runs), then each operand in turn 4
    bytes past a 16-byte boundary: one such operand sends the call down the scalar kernel, with the same values.
    Transcendental ops are allowed 4 x the float32 restatement's error on these inputs; measured over the six sizes: powerlaw 1.7 (powf)
    2.6e-6, powerlaw 0.5 (sqrtf) 6.3e-8, laplace_add_ (log1pf) 1.1e-6.  The project tolerance is the larger bound almost everywhere."""
    count, run, ref, transcendental = LAYOUT_OPS[name]
    cpu = _layout_inputs(name, count, n)
    want = ref(d64(*cpu))
    floor = 4 * R.ref32_error(lambda *a: ref(list(a)), *d64(*cpu)) if transcendental else 0.0
    print(f"{name} n={n}: float32 restatement error {floor / 4:.3e}")
    for which in range(-1, count):
        got = run(hl, [put(t, 1 if k == which else 0) for k, t in enumerate(cpu)])
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g is None) == (w is None), (name, which)
            if w is not None:
                R.within(g, w, floor=floor)


@pytest.mark.parametrize("n", NS)
def test_apply_norm_sizes_and_alignment(hl, n):
    """sonar_norm_decision_f32 + sonar_apply_norm_f32 against the float64 decision and (x - mean) / std * factor."""
    norm, dec = _norm_for_layout(hl)
    got = norm.cpu()
    torch.testing.assert_close(got[:2].double(), torch.tensor(dec[:2], dtype=torch.float64), rtol=R.RTOL, atol=R.ATOL)
    torch.testing.assert_close(got[2].double(), torch.tensor(1.0 / dec[1], dtype=torch.float64), rtol=R.RTOL, atol=R.ATOL)
    assert got[3].item() == R.f32(dec[4]) and got[4:].view(torch.int32).tolist() == [int(dec[2]), int(dec[3])] == [1, 1]
    x = seeded(n, seed=n, scale=1.7, shift=0.4)
    want = R.apply_norm(x.double(), dec)
    for off in (0, 1):
        R.within(hl.apply_norm_(put(x, off), norm), want)


@pytest.mark.parametrize("n", NS)
def test_axpby_stats_sizes_alignment_and_partials(hl, n):
    """y*ymul + x*xmul, a multiplier of exactly 1 included, and the (sum, sum of squares) partials: every one of the NPART slots is
    written (the buffer starts as NaN), and they add up to the float64 sums of the stored result."""
    y, x = seeded(n, seed=n + 1), seeded(n, seed=n + 2)
    for ymul, xmul in ((1.0, 0.37), (-0.5, 1.0)):
        want, _s, _q = R.axpby(y.double(), R.f32(ymul), x.double(), R.f32(xmul))
        for which in (-1, 0, 1):  # a misaligned operand: the wrapper's axpby_ + stats pair
            part = nan_partials(hl)
            got, part = hl.axpby_stats_(put(y, int(which == 0)), ymul, put(x, int(which == 1)), xmul, part)
            R.within(got, want)
            sums, own = part.view(-1, 2).sum(0).cpu(), got.double().cpu()
            # float64 sums in another order: at most n roundings of 2^-53 relative to the sum of magnitudes
            torch.testing.assert_close(sums, torch.stack([own.sum(), (own * own).sum()]), rtol=0, atol=n * 2.0**-53 * float((own * own).sum() + own.abs().sum()) + 1e-300)


# ================================================================================================ the step kernels
STEP_CFGS = CFGS + [
    orc.MomentumCfg(init="RAND"),
    orc.MomentumCfg(init="RAND", mode="DENOISED"),  # the only mode in which a FRESH history must not be mixed into the prediction
    orc.MomentumCfg(momentum_start_step=1, momentum_end_step=1, always_update_history=True),  # steps 0, 2: use_momentum 0, update_hist 1
    orc.MomentumCfg(mode="CLASSIC", momentum_start_step=1, momentum_end_step=1, always_update_history=True),
    orc.MomentumCfg(momentum_start_step=1, momentum_end_step=1, always_update_history=False, init="SAMPLE"),
]
SIGMAS = [7.0, 4.0, 2.0, 1.0]
NOISE_VARIANTS = [None, "plain", "shift_and_scale", "scale_only", "as_is"]
# (shape, operand x misaligned?)
STEP_LAYOUTS = [((2, 4, 8, 8), False), ((1, 3, 7, 5), False), ((1, 3, 7, 5), True)]


def _cfg_id(c):
    return f"{c.mode}-{c.init}-{c.blend_mode}-m{c.momentum}-h{c.momentum_hist}-d{c.direction}-s{c.momentum_start_step}-a{int(c.always_update_history)}"


def _model(x):
    return x * 0.5 + torch.tanh(x) * 0.1


def _noise(hl, variant, shape, seed):
    """(device noise, device noise_norm or None, float64 noise, float64 decision or None) of a variant."""
    if variant is None:
        return None, None, None, None
    if variant == "plain":
        nz = seeded(*shape, seed=seed)
        return nz.cuda(), None, nz.double(), None
    nz, factor = R.norm_noise(variant, shape, seed=seed)
    nd = nz.cuda()
    norm = hl.norm_decision(hl.stats(nd), nz.numel(), factor)
    assert norm.cpu()[4:].view(torch.int32).tolist() == [int(v) for v in R.NORM_OUTCOMES[variant]], variant
    return nd, norm, nz.double(), R.norm_decision(nz.double(), factor)


def _check(got, want, what):
    assert (got is None) == (want is None), f"{what}: the kernel {'returns no' if got is None else 'returns a'} tensor, the reference the opposite"
    if want is not None:
        R.within(got, want)


def _round(t):
    return None if t is None else t.float()


@pytest.mark.parametrize("layout", STEP_LAYOUTS, ids=lambda l: f"{'x'.join(map(str, l[0]))}{'-misaligned' if l[1] else ''}")
@pytest.mark.parametrize("cfg", STEP_CFGS, ids=_cfg_id)
def test_euler_kernel_three_steps_every_variant(hl, cfg, layout):
    """sonar_momentum_euler_f32: three consecutive steps (no history -> created -> updated) for every noise variant; x_out and the history
    against the float64 MomentumState, and whether a history exists at all.  Both sides start every step from the same float32 values (the
    reference's results, rounded), so one kernel launch is compared at a time."""
    shape, misaligned = layout
    rand = cfg.init == "RAND"
    for variant in NOISE_VARIANTS:
        x = seeded(*shape, seed=9)
        h = seeded(*shape, seed=19) if rand else None
        for step in range(3):
            den = _model(x)
            fresh = rand and step == 0
            nd, norm, n64, dec = _noise(hl, variant, shape, seed=30 + step)
            kc = make_cfg(hl, cfg, orc.MomentumState(cfg), step, h is not None, fresh)
            dt = SIGMAS[step + 1] - SIGMAS[step]
            want_x, want_h = R.euler_step(cfg, step, *d64(x, den, h), SIGMAS[step], dt, noise=n64, noise_scale=NSCALE, norm=dec, h_fresh=fresh)
            got_x, got_h = hl.momentum_euler(put(x, int(misaligned)), den.cuda(), None if h is None else h.cuda(), kc, SIGMAS[step], dt, noise=nd,
                                             noise_scale=NSCALE, noise_norm=norm)
            _check(got_x, want_x, "x_out")
            _check(got_h, want_h, f"history after step {step}")
            if not cfg.always_update_history and step < cfg.momentum_start_step:
                assert got_h is None and kc.update_hist == 0 and kc.use_momentum == 0  # outside the window: nothing is produced, `present` is 0
            if cfg.always_update_history and not (cfg.momentum_start_step <= step <= cfg.momentum_end_step):
                assert (kc.use_momentum, kc.update_hist) == (0, 1) and got_h is not None
            x, h = _round(want_x), _round(want_h)


@pytest.mark.parametrize("layout", STEP_LAYOUTS, ids=lambda l: f"{'x'.join(map(str, l[0]))}{'-misaligned' if l[1] else ''}")
@pytest.mark.parametrize("cfg", STEP_CFGS, ids=_cfg_id)
def test_dpmpp_kernels_three_steps_every_variant(hl, cfg, layout):
    """sonar_dpmpp_stage1_f32 -> model -> sonar_dpmpp_stage2_f32, three consecutive steps, adj_is_one on and off, every noise variant:
    x2, md1 and the history after stage 1; x_out, dd and the history after stage 2; x_out identical with and without dd."""
    shape, misaligned = layout
    rand = cfg.init == "RAND"
    sig64 = torch.tensor(SIGMAS, dtype=torch.float64)
    for adj_is_one in (False, True):
        for variant in NOISE_VARIANTS:
            x = seeded(*shape, seed=9)
            h = seeded(*shape, seed=19) if rand else None
            for step in range(3):
                k = {key: R.f32(v) for key, v in R.dpmpp_scalars(sig64[step], sig64[step + 1], 0.9, 1.05).items()}
                fresh = rand and step == 0
                den = _model(x)
                nd, norm, n64, dec = _noise(hl, variant, shape, seed=40 + step)
                kc = make_cfg(hl, cfg, orc.MomentumState(cfg), step, h is not None, fresh)
                want = R.dpmpp_stage1(cfg, step, *d64(x, den, h), k["sigma"], k["expm1_a"], k["ratio_a"], adj_is_one, noise=n64,
                                      noise_scale=k["noise_scale_a"], norm=dec, h_fresh=fresh)
                got = hl.dpmpp_stage1(put(x, int(misaligned)), den.cuda(), None if h is None else h.cuda(), kc, k["sigma"], k["expm1_a"], k["ratio_a"],
                                      adj_is_one, noise=nd, noise_scale=k["noise_scale_a"], noise_norm=norm)
                for g, w, what in zip(got, want, ("x2", "md1", f"history after stage 1 of step {step}")):
                    _check(g, w, what)
                x2, md1, h = (_round(t) for t in want)
                den2 = _model(x2)
                nd, norm, n64, dec = _noise(hl, variant, shape, seed=50 + step)
                kc = make_cfg(hl, cfg, orc.MomentumState(cfg), step, h is not None)
                want = R.dpmpp_stage2(cfg, step, *d64(x, den2, md1, h), k["sigma_s"], k["expm1_b"], k["ratio_b"], FAC, adj_is_one, noise=n64,
                                      noise_scale=k["noise_scale_b"], norm=dec)
                args = (put(x, int(misaligned)), den2.cuda(), md1.cuda(), None if h is None else h.cuda(), kc, k["sigma_s"], k["expm1_b"], k["ratio_b"], FAC,
                        adj_is_one)
                got = hl.dpmpp_stage2(*args, noise=nd, noise_scale=k["noise_scale_b"], noise_norm=norm, want_dd=True)
                for g, w, what in zip(got, want, ("x_out", "dd", f"history after stage 2 of step {step}")):
                    _check(g, w, what)
                bare = hl.dpmpp_stage2(*args, noise=nd, noise_scale=k["noise_scale_b"], noise_norm=norm, want_dd=False)
                assert bare[1] is None and torch.equal(bare[0], got[0]) and (bare[2] is None) == (got[2] is None)
                if got[2] is not None:
                    assert torch.equal(bare[2], got[2])
                x, h = _round(want[0]), _round(want[2])


def test_euler_kernel_beyond_the_streaming_store_threshold(hl):
    """n = 8 Mi + 7 with aligned operands: EulerOpT<true> (non-temporal stores, taken above 8 Mi elements) and its scalar tail, with
    history in and out and noise."""
    n = 8 * 2**20 + 7
    cfg = orc.MomentumCfg(mode="CLASSIC", momentum=0.8, momentum_hist=0.5, direction=1.5)
    gen = torch.Generator().manual_seed(77)
    x, den, h, nz = (torch.randn(n, generator=gen) for _ in range(4))
    kc = make_cfg(hl, cfg, orc.MomentumState(cfg), 1, True)
    ops = [t.cuda() for t in (x, den, h, nz)]
    assert all(t.data_ptr() % 16 == 0 for t in ops)
    got_x, got_h = hl.momentum_euler(ops[0], ops[1], ops[2], kc, SIG, DT, noise=ops[3], noise_scale=NSCALE)
    got_x, got_h = got_x.cpu(), got_h.cpu()
    chunk = 1 << 21
    for a in range(0, n, chunk):  # (the float64 reference in pieces: a quarter of a GiB at a time instead of two)
        s = slice(a, min(n, a + chunk))
        want_x, want_h = R.euler_step(cfg, 1, *d64(x[s], den[s], h[s]), SIG, DT, noise=nz[s].double(), noise_scale=NSCALE)
        R.within(got_x[s], want_x)
        R.within(got_h[s], want_h)


# ================================================================================================ reductions over a middle axis
MID_VIEWS = [(3, 4, 35), (5, 3, 257), (1, 16, 1)]


def test_std_mid(hl):
    """Unbiased std over the middle axis of every view, of 1000 + N(0, 1) (a one-pass float32 sum of squares is useless there), and
    mid == 1, where every output is NaN like torch.std's (those 16 outputs are the exclusion: 0.6 % of this test's outputs)."""
    got, want = [], []
    for k, view in enumerate(MID_VIEWS + [(5, 3, 257), (2, 1, 8)]):
        x = seeded(*view, seed=k, shift=1000.0 if k == 3 else 0.0)
        out = hl.std_mid(x.cuda(), *view)
        assert out.numel() == view[0] * view[2]
        got.append(out.cpu().reshape(-1))
        want.append(R.std_mid(x.double()).reshape(-1))
    want = torch.cat(want)
    planned = torch.zeros(want.numel(), dtype=torch.bool)
    planned[-16:] = True
    R.within(torch.cat(got), want, exclude=planned)


@pytest.mark.parametrize("use_abs", [False, True])
@pytest.mark.parametrize("view", MID_VIEWS)
def test_amax_mid(hl, view, use_abs):
    x = seeded(*view, seed=3)
    assert torch.equal(hl.amax_mid(x.cuda(), *view, use_abs).cpu().reshape(view[0], view[2]), R.amax_mid(x, use_abs))
    neg = -x.abs() - 0.5  # all negative: the maximum must not be clipped at 0 (nor start from it)
    got = hl.amax_mid(neg.cuda(), *view, use_abs).cpu().reshape(view[0], view[2])
    assert torch.equal(got, R.amax_mid(neg, use_abs)) and bool((got < 0).all()) != use_abs


@pytest.mark.parametrize("use_abs", [False, True])
def test_amax_mid_propagates_a_nan_to_its_own_output_only(hl, use_abs):
    view = (5, 3, 257)
    x = seeded(*view, seed=4)
    x[3, 1, 200] = float("nan")
    got = hl.amax_mid(x.cuda(), *view, use_abs).cpu().reshape(5, 257)
    nan = torch.isnan(got)
    assert int(nan.sum()) == 1 and bool(nan[3, 200]) and nan.numel() > 100
    assert same_values(got, R.amax_mid(x, use_abs))


@pytest.mark.parametrize("use_abs", [False, True])
@pytest.mark.parametrize("mid", [1000, 8192])
def test_amax_mid_row_kernels(hl, mid, use_abs):
    """inner == 1: one workgroup per row, 256 threads below 8192 elements and 1024 from there; rows of all-negative values, a NaN in
    one row of 128."""
    rows = 128
    x = seeded(rows, mid, 1, seed=mid)
    x[5] = -x[5].abs() - 0.25
    assert torch.equal(hl.amax_mid(x.cuda(), rows, mid, 1, use_abs).cpu(), R.amax_mid(x, use_abs).reshape(-1))
    x[77, mid - 3, 0] = float("nan")
    got = hl.amax_mid(x.cuda(), rows, mid, 1, use_abs).cpu()
    assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[77])) and same_values(got, R.amax_mid(x, use_abs).reshape(-1))


@pytest.mark.parametrize("view", MID_VIEWS)
def test_div_mid(hl, view):
    x = seeded(*view, seed=5)
    d = seeded(view[0], view[2], seed=6).abs() + 0.5
    R.within(hl.div_mid_(x.cuda(), *view, d.cuda()), R.div_mid(x.double(), d.double()))


@pytest.mark.parametrize("follow_sign", [False, True])
@pytest.mark.parametrize("inner", [1, 7])
def test_mul_table(hl, inner, follow_sign):
    """A table of 4 entries over 10 rows (the table wraps and does not divide the row count); with follow_sign the results take the sign
    of 1 - s: negative for the entry 2.5, and for the entry that is exactly 1 a positive zero, so those results are non-negative."""
    table = torch.tensor([0.5, 1.0, 2.5, -1.5])
    x = seeded(10 * inner, seed=7)
    got = hl.mul_table_(x.cuda(), table.cuda(), inner, follow_sign).cpu()
    R.within(got, R.mul_table(x.double(), table.double(), inner, follow_sign))
    ones = ((torch.arange(x.numel()) // inner) % 4) == 1
    if follow_sign:
        assert torch.equal(got[ones], x[ones].abs()) and not bool(torch.signbit(got[ones]).any())
    else:
        assert torch.equal(got[ones], x[ones])


@pytest.mark.parametrize("op", [0, 1])
def test_row_affine(hl, op):
    x, a, b = seeded(6, 37, seed=8), seeded(6, seed=9), seeded(6, seed=10).abs() + 0.5
    R.within(hl.row_affine(op, x.cuda(), 6, 37, a.cuda(), b.cuda()), R.row_affine(op, *d64(x, a, b)))


@pytest.mark.parametrize("p", [0.5, 1.0, 2.0, 1.7])
def test_clamp_signpow_rows(hl, p):
    """copysign(|clamp(x, -lim, lim)|^p, x) with lim = limit[row] * 0.9, a row whose limit is 0 (every result a zero), and -0.0 / 0.0
    inputs, whose sign survives.  p = 1.7 is powf, allowed 4 x the float32 restatement's error (measured 2.2e-7; 8.0e-8, 6.0e-8
    and 8.5e-7 at p = 0.5, 1 and 2, which are special-cased like ATen's pow), never less than the project tolerance."""
    x = seeded(5, 37, seed=11, scale=2.0)
    x[1, 3], x[1, 4], x[3, 0] = -0.0, 0.0, -0.0
    limit = torch.tensor([1.5, 0.7, 0.0, 2.5, 10.0])
    want = R.clamp_signpow_rows(x.double(), limit.double(), R.f32(0.9), R.f32(p))
    floor = 4 * R.ref32_error(R.clamp_signpow_rows, x.double(), limit.double(), R.f32(0.9), R.f32(p))
    print(f"clamp_signpow_rows p={p}: float32 restatement error {floor / 4:.3e}")
    got = hl.clamp_signpow_rows_(x.cuda(), 5, 37, limit.cuda(), 0.9, p).cpu()
    R.within(got, want, floor=floor)
    assert bool((got[2] == 0).all())
    zero = x == 0
    zero[2] = False
    assert torch.equal(torch.signbit(got[zero]), torch.signbit(x[zero])) and bool((got[zero] == 0).all())
    live = x != 0
    live[2] = False  # (clamped between -0.0 and 0.0: which zero a minimum of the two returns is not defined)
    assert torch.equal(torch.signbit(got[live]), torch.signbit(x[live]))


# ================================================================================================ bcast_gain / ratio_mix
@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("bcast", [0, 1, 2])
@pytest.mark.parametrize("view", [(2, 3, 35), (1, 17, 181)], ids=["one-block", "3x1024+5"])
def test_bcast_gain_and_ratio_mix(hl, view, bcast, store):
    """v = x k (1 / (std |strength| + 1) + 1) with the std vector of each broadcast mode holding a distinct value per index (a wrong
    stride changes the answer); the partials start as NaN, so every NPART slot must be written, and add up to (sum x^2, sum v^2);
    ratio_mix then reads its ratio from them."""
    outer, mid, inner = view
    assert outer * mid * inner in (210, 3 * 1024 + 5)
    x = seeded(*view, seed=12)
    nstd = outer * (1 if bcast == 0 else mid if bcast == 1 else inner)
    stdv = 0.1 + 0.013 * torch.arange(nstd, dtype=torch.float32)
    strength, k = R.f32(0.6), R.f32(1.3)
    want, sx, sv = R.bcast_gain(x.double(), stdv.double(), bcast, strength, k)
    part = nan_partials(hl)
    got, part = hl.bcast_gain(x.cuda(), stdv.cuda(), outer, mid, inner, bcast, strength, k, store=store, partials=part)
    assert (got is not None) == store
    sums = part.view(-1, 2).sum(0).cpu()
    torch.testing.assert_close(sums[0], sx, rtol=1e-12, atol=0)  # float64 sums of exact float32 products
    torch.testing.assert_close(sums[1], sv, rtol=R.RTOL, atol=R.ATOL)
    if store:
        R.within(got, want)
        torch.testing.assert_close(sums[1], (got.double() ** 2).sum().cpu(), rtol=1e-12, atol=0)
    a = want.float()
    mixed = hl.ratio_mix(a.cuda(), -0.6, x.cuda(), 1.6, part, float(k) * float(k), part)
    R.within(mixed, R.ratio_mix(a.double(), R.f32(-0.6), x.double(), R.f32(1.6), sx, float(k) * float(k), sv))


# ================================================================================================ rescales
@pytest.mark.parametrize("targets", [(0.1, 0.3), (-1.5, 2.0)])
def test_minmax_rescale(hl, targets):
    """normalize_to_scale's tail: a constant row (the denominator is eps alone), a NaN (kept: 1 of 148 elements, 0.7 %), and with (0.1, 0.3)
    the span that is rounded once from double -- visible only bit for bit, so that case is also compared with the float32 run of the
    restatement (every step an IEEE operation rounded on its own, as in the kernel)."""
    x = seeded(4, 37, seed=13)
    x[1] = 0.625
    lo, hi = x.amin(1), x.amax(1)
    x[2, 5] = float("nan")
    planned = torch.isnan(x)
    got = hl.minmax_rescale(x.cuda(), 4, 37, lo.cuda(), hi.cuda(), 1e-7, *targets).cpu()
    R.within(got, R.minmax_rescale(*d64(x, lo, hi), R.f32(1e-7), *targets), exclude=planned)
    assert torch.equal(got[1], torch.full((37,), targets[0]))
    if targets == (0.1, 0.3):
        assert same_values(got, R.minmax_rescale(x, lo, hi, 1e-7, *targets))


def test_signed_rescale_fixture_rows(hl):
    """The rows and target sets of tests/golden/signed_rescale.npz (mixed, one-signed, with zeros; fixed and data-derived targets, either
    sign skipped): against the float64 restatement and the reference's own outputs; a skipped sign and the zeros exactly."""
    rows, names, cases = R.load_signed_rescale_golden()
    for name, (targets, golden_out) in cases.items():
        got = hl.signed_rescale(rows.cuda(), rows.shape[0], rows.shape[1], *targets).cpu()
        R.within(got, R.signed_rescale(rows.double(), *targets))
        R.within(got, golden_out.double())
        assert bool((got[rows == 0] == 0).all()), name
        if name == "skip_neg":
            assert torch.equal(got[rows < 0], rows[rows < 0])
        if name == "skip_pos":
            assert torch.equal(got[rows > 0], rows[rows > 0])


def test_signed_rescale_row_loop_and_nan(hl):
    """4100 rows of 5: more rows than the statistics pass has workgroups (4096), so its row loop runs; a NaN input comes out 0."""
    x = seeded(4100, 5, seed=14)
    x[::7, 2] = 0.0
    x[4099] = torch.tensor([-1.0, -2.0, -3.0, -0.5, -4.0])
    x[4098] = torch.tensor([1.0, 2.0, 3.0, 0.5, 4.0])
    x[4097, 1] = float("nan")
    targets = (-4.3, 0.0, -1.0, 3.7)
    got = hl.signed_rescale(x.cuda(), 4100, 5, *targets).cpu()
    assert got[4097, 1].item() == 0.0 and not bool(torch.isnan(got).any())
    R.within(got, R.signed_rescale(x.double(), *targets))
    assert bool((got[x == 0] == 0).all())


# ================================================================================================ spectral helpers
@pytest.mark.parametrize("inner", [1, 33])
@pytest.mark.parametrize("C", [1, 3, 16, 64])
def test_cdft_mid(hl, C, inner):
    """DFT along the middle axis against torch.fft in complex128: forward from complex and from real input, inverse (x C, no 1 / C) to
    complex and to real output.  sincospif twiddles summed over C terms: 4 x the error of the complex64 torch.fft on the same input
    (measured, worst of the four directions and both inner sizes: 0 at C = 1, 4.0e-7 at C = 3, 1.2e-6 at C = 16, 3.3e-6 at C = 64), never
    less than the project tolerance."""
    outer = 2
    zr, zi = seeded(outer, C, inner, seed=15), seeded(outer, C, inner, seed=16)
    z = torch.complex(zr, zi)
    for src, inverse, real_out in ((z, False, False), (zr, False, False), (z, True, False), (z, True, True)):
        src64 = src.to(torch.complex128 if src.is_complex() else torch.float64)
        want = R.cdft_mid(src64, inverse, real_out)
        floor = 4 * R.ref32_error(R.cdft_mid, src64, inverse, real_out)
        print(f"cdft_mid C={C} inner={inner} inverse={inverse} real_in={not src.is_complex()} real_out={real_out}: float32 restatement error {floor / 4:.3e}")
        got = hl.cdft_mid(src.cuda(), outer, C, inner, inverse=inverse, real_out=real_out)
        assert got.dtype == (torch.float32 if real_out else torch.complex64)
        if real_out:
            R.within(got, want, floor=floor)
        else:
            R.within(torch.view_as_real(got), torch.view_as_real(want), floor=floor)


def test_cdft_mid_refuses_what_it_cannot_run(hl):
    lib = hl.load()
    st = torch.cuda.current_stream().cuda_stream
    z = torch.full((2 * 65 * 4 * 2,), 7.0, device="cuda")
    out = torch.full_like(z, 5.0)
    assert lib.sonar_cdft_mid_f32(z.data_ptr(), out.data_ptr(), 2, 65, 4, 0, 0, 0, st) == hl.ERR_ARG and b"sonar_cdft_mid_f32" in lib.sonar_last_error()
    assert lib.sonar_cdft_mid_f32(z.data_ptr(), out.data_ptr(), 2, 0, 4, 0, 0, 0, st) == hl.ERR_ARG
    assert lib.sonar_cdft_mid_f32(z.data_ptr(), z.data_ptr(), 2, 4, 4, 0, 0, 0, st) == hl.ERR_ARG  # in place
    with pytest.raises(hl.SonarHipError, match="code -1"):
        hl.cdft_mid(torch.zeros(2, 65, 4, dtype=torch.complex64, device="cuda"), 2, 65, 4, inverse=False)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((out == 5.0).all())  # nothing was launched


@pytest.mark.parametrize("half", [True, False], ids=["half", "full"])
@pytest.mark.parametrize("hw", [(4, 6), (5, 7)])
@pytest.mark.parametrize("C", [1, 3])
def test_spectral_logamp(hl, C, hw, half):
    """la = log|z| of the spectrum handed in, and `full` = |log|F x|| at every bin of the full spectrum of the real input x -- over (H, W),
    and over (C, H, W) for C = 3, where a dropped column's Hermitian partner sits at channel (C - c) % C.  logf: 4 x the float32
    restatement's error (measured 8.6e-8 ... 1.5e-7 over the eight cases: the project tolerance is the larger bound)."""
    H, W = hw
    B = 2
    x = seeded(B, C, H, W, seed=17)
    spec = R.spectrum_of(x.double(), C > 1)
    Wz = W // 2 + 1 if half else W
    z = spec[..., :Wz].to(torch.complex64).contiguous()
    want_la = R.logamp(z.to(torch.complex128))
    floor = 4 * R.ref32_error(R.logamp, z.to(torch.complex128))
    print(f"spectral_logamp C={C} {H}x{W} half={half}: float32 restatement error {floor / 4:.3e}")
    la, full = hl.spectral_logamp(z.cuda().reshape(B * C, H, Wz), B * C, C, H, W)
    R.within(la.reshape(B, C, H, Wz), want_la, floor=floor)
    R.within(full.reshape(B, C, H, W), R.full_abs_logamp(x.double(), C > 1), floor=floor)


@pytest.mark.parametrize("channel_sym", [False, True])
@pytest.mark.parametrize("nq", [1, 3])
def test_spectral_signum_mask(hl, nq, channel_sym):
    """z *= gain * (mult_low * mult_high) ^ intensity with one quantile row, or one per channel (and their symmetrised pair): bins below
    q_low / 2 (the low clamp at 0.5), between the quantiles, above q_high, and beyond q_max (the high clamp at 0.5) are all present.
    powf: 4 x the float32 restatement's error (measured 1.4e-7 ... 2.1e-7 over the four cases), never less than the project tolerance."""
    B, C, elems = 2, 3, 20
    q = torch.tensor([[2.0, 4.0, 6.0], [1.5, 3.5, 7.0], [2.5, 5.0, 5.5]])[:nq].contiguous()
    la = (torch.arange(B * C * elems, dtype=torch.float32).reshape(B * C, elems) * 0.37) % 8.0 + 0.05
    for ql, qh, qm in q.tolist():
        assert bool((la < ql / 2).any()) and bool(((la > qh) & (la < qh + (qm - qh) / 2)).any()) and bool((la > qm).any()) and bool(((la > ql) & (la < qh)).any())
    z = torch.complex(seeded(B * C, elems, seed=18), seeded(B * C, elems, seed=19))
    intensity, gain = R.f32(1.3), R.f32(0.7)
    args64 = (z.to(torch.complex128), la.double(), q.double(), C, intensity, gain, channel_sym)
    want = R.spectral_signum_mask(*args64)
    floor = 4 * R.ref32_error(R.spectral_signum_mask, *args64)
    print(f"spectral_signum_mask nq={nq} channel_sym={channel_sym}: float32 restatement error {floor / 4:.3e}")
    got = hl.spectral_signum_mask_(z.cuda(), la.cuda(), q.cuda(), B * C, C, elems, intensity, gain, channel_sym)
    R.within(torch.view_as_real(got), torch.view_as_real(want), floor=floor)
