"""SonarApplyLatentOperationCFG's arithmetic around the operations (prediction flip, t2, lerp): the two fused launches
(hip_lib.cfg_op_prepare / cfg_op_finish) against the same arithmetic composed from the library's other elementwise calls on the same
tensors -- to_d x 2 + subtract before the operations (3 launches), add + mul_scalar + subtract + blend after them (4 launches).  The
composition has one scalar sigma only (to_d / mul_scalar take a scalar), so both columns run with a one-element sigma; the fused calls are
timed with a per-sample sigma as well.  No timed call writes a tensor another one reads: every window runs on the data that was compared
before the timing.  fp32, HIP events; the variants of a stage take turns, window by window (2000 calls after 100 warm-up calls each),
five rounds, median / min per variant; both sides allocate their outputs from torch's caching allocator.
Usage: python scratch/cfg_op_time.py [output file; default profiles/cfg_op_time.txt]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
lines = ["# scratch/cfg_op_time.py on one MI355X (fp32, flip + t2 + lerp 0.5, HIP events, 5 alternating windows of 2000 calls per variant)"]
SIGMA, W = 3.7, 0.5


def report(variants, iters=2000, warm=100, rounds=5):
    """variants: [(name, fn)]; their windows alternate, so a drift of the machine meets every variant alike.  Returns the medians."""
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(bench.event_us(fn, iters, warm))
    meds = []
    for name, _ in variants:
        t = sorted(times[name])
        meds.append(t[len(t) // 2])
        lines.append(f"{name:86s} median {meds[-1]:8.2f} us  min {t[0]:8.2f}  max {t[-1]:8.2f}")
        print(lines[-1], flush=True)
    return meds


def composed_prepare(x, t1, t2):
    f1, f2 = hl.to_d(x, t1, SIGMA), hl.to_d(x, t2, SIGMA)
    return hl.blend("subtract_b", f1, f2, 1.0), f2


def composed_finish(result, t2f, x, t1_orig):
    r = hl.blend("inject", result, t2f, 1.0)  # result + t2f into a new tensor (3N, what axpby_ moves in place)
    r = hl.mul_scalar(r, SIGMA, out=r)
    r = hl.blend("subtract_b", x, r, 1.0, out=r)
    return hl.blend("lerp", t1_orig, r, W)


for shape in ((2, 4, 128, 128), (16, 16, 128, 128)):
    x, t1, t2 = (torch.randn(shape, device="cuda") for _ in range(3))
    one = torch.tensor([SIGMA], device="cuda")
    per = torch.full((shape[0],), SIGMA, device="cuda")
    n = x.numel()
    res, t2f = hl.cfg_op_prepare(x, t1, t2, one)
    cres, ct2f = composed_prepare(x, t1, t2)
    assert torch.equal(res, cres) and torch.equal(t2f, ct2f), "prepare: fused and composed differ"
    fused_out = hl.cfg_op_finish(res, t2f, x, one, t1, "lerp", W)
    comp_out = composed_finish(res, t2f, x, t1)
    torch.testing.assert_close(fused_out, comp_out, rtol=4e-6, atol=4e-6 * float(fused_out.abs().max()))
    same = "bit-equal" if torch.equal(fused_out, comp_out) else f"max difference {float((fused_out - comp_out).abs().max()):.2e}"
    keep = [t.clone() for t in (x, t1, t2, res, t2f)]
    tag = "x".join(map(str, shape))
    lines.append(f"## {tag}: {n} values, {n * 4 / 1e6:.1f} MB per tensor; fused and composed results: prepare bit-equal, finish {same}")
    fp, _, cp = report([(f"{tag}: prepare, fused (1 launch, 5N values moved), one sigma", lambda: hl.cfg_op_prepare(x, t1, t2, one)),
                        (f"{tag}: prepare, fused, per-sample sigma", lambda: hl.cfg_op_prepare(x, t1, t2, per)),
                        (f"{tag}: prepare, composed (3 launches, 9N)", lambda: composed_prepare(x, t1, t2))])
    ff, _, cf = report([(f"{tag}: finish, fused (1 launch, 5N), one sigma", lambda: hl.cfg_op_finish(res, t2f, x, one, t1, "lerp", W)),
                        (f"{tag}: finish, fused, per-sample sigma", lambda: hl.cfg_op_finish(res, t2f, x, per, t1, "lerp", W)),
                        (f"{tag}: finish, composed (4 launches, 11N)", lambda: composed_finish(res, t2f, x, t1))])
    assert all(torch.equal(a, b) for a, b in zip((x, t1, t2, res, t2f), keep)), "a timed call wrote an input"
    lines.append(f"{tag}: both stages, one sigma: fused {fp + ff:.2f} us, composed {cp + cf:.2f} us ({(cp + cf) / (fp + ff):.2f}x); "
                 f"fused bandwidth {5 * n * 4 / fp / 1e6:.2f} / {5 * n * 4 / ff / 1e6:.2f} TB/s")
    print(lines[-1], flush=True)
    del x, t1, t2, res, t2f, cres, ct2f, fused_out, comp_out, keep

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cfg_op_time.txt")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
