"""SonarNoiseImage on a 4 x 1024 x 1024 x 3 fp32 image that already lives on the device, gaussian noise, generate mode (cpu_noise=False):
us per node call in clamp and in rescale mode, the part of it that is the image side (extremes of the noise + the compose launch, + the
in-place rescale), the same for 4 channels, and a copy_ of the same image for scale.  HIP events, median / min of 5 x 10 calls.
Usage: python scratch/image_noise_time.py [output file; default profiles/r08_image_noise_time.txt]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
reg = importlib.import_module("comfyui_sonar_amd.py.nodes.registry")
node = reg.NODE_CLASS_MAPPINGS["SonarNoiseImage"]
sockets = {k: v["default"] for k, v in reg.NODE_ABI["SonarNoiseImage"]["inputs"].items() if "default" in v}
sockets.update(noise_type="gaussian", cpu_noise=False, seed=1)
lines = ["# scratch/image_noise_time.py on one MI355X (image on the device, gaussian, generate mode, fp32, HIP events, median / min of 5 x 10 calls)"]


def report(name, fn, iters=10, warm=2):
    fn()
    times = sorted(bench.event_us(fn, iters, warm) for _ in range(5))
    lines.append(f"{name:64s} median {times[2]:9.1f} us  min {times[0]:9.1f}")
    print(lines[-1], flush=True)


for channels in (3, 4):
    shape = (4, 1024, 1024, channels)
    image = torch.rand(shape, device="cuda")
    dst = torch.empty_like(image)
    mb = image.numel() * 4 / 1e6
    mode = "RGB" if channels == 3 else "RGBA"
    report(f"{shape}: copy_ of the image ({mb:.1f} MB read + written)", lambda: dst.copy_(image))
    for overflow in ("clamp", "rescale"):
        report(f"{shape}: node call, {overflow}", lambda: node.go(**dict(sockets, image=image, overflow_mode=overflow, channel_mode=mode)))
    noise = torch.randn((4, channels, 1024, 1024), device="cuda")
    mask = (1 << channels) - 1

    def image_side(rescale, noise=noise, image=image, shape=shape, mask=mask):
        lo, hi = hl.minmax_rows(noise, 4, noise.numel() // 4)
        out = hl.image_noise_compose(noise, image, shape, noise_lo=lo, noise_hi=hi, multiplier=0.5, channel_mask=mask, clamp=not rescale)
        return hl.image_rescale_(*out) if rescale else out

    def compose_only(lo, hi, noise=noise, image=image, shape=shape, mask=mask):
        return hl.image_noise_compose(noise, image, shape, noise_lo=lo, noise_hi=hi, multiplier=0.5, channel_mask=mask)

    lo, hi = hl.minmax_rows(noise, 4, noise.numel() // 4)
    report(f"{shape}: image side, clamp (extremes + compose)", lambda: image_side(False))
    report(f"{shape}: image side, rescale (extremes + compose + rescale)", lambda: image_side(True))
    report(f"{shape}: compose launch alone, clamp", lambda: compose_only(lo, hi))
    report(f"{shape}: extremes of the noise alone (sonar_minmax_rows_f32)", lambda: hl.minmax_rows(noise, 4, noise.numel() // 4))
    del image, dst, noise

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_image_noise_time.txt")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
