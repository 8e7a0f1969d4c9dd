"""The call sites of the general-size power-noise plane kernel (csrc/power_any_core.h), as the library itself plans them.

For a plane size the host picks a kernel family, a factor pair per axis, whether the inverse rows fold the c2r pre-twiddle into their
first pass, and the workgroup size; each choice selects separately inlined code.  ``sonar_power_any_plan`` reports those choices through
the helpers the launch calls, so nothing here restates ``best_split``, ``any_needs_all`` or the ``c2r_fuse`` rule.

A SITE is one of
    (family, "cols" | "rows", pass, how)          how = the codelet length, "direct" (direct sums), "direct1" (direct sums of a single
                                                  term: the first pass of a line with no codelet factor, or of a line of one value),
                                                  "absent" (a second pass of length 1)
    (family, "rows", 0, how, "fold" | "pre", n)   the inverse rows' first pass: pre-twiddle folded in, taken in n row batches, or a pass
                                                  of its own before it (n = 0); the forward rows of the spectral filter run the same
                                                  (how) in forward form
    (family, "threads", 512 | 1024)
with family "small" (run-time sizes, codelets 2 .. 12), "all" (every codelet length) or "bucket HxW" -- each SDXL bucket is a kernel of
its own, so each is a family of its own here.  ``SWEEP`` is a committed list of plane sizes that reaches every site that exists over
the whole accepted domain (tests/test_power_any_sites_cpu.py holds it to that); tests/test_gpu_power_any_sites.py runs every mode of
the kernel at those sizes against an fp64 DFT.

``python -m tests.power_any_sites`` prints a fresh ``SWEEP`` (``greedy_cover``) after a change to the plan rules or the codelet sets.
"""
import ctypes as C

H_MAX, W_MAX = 512, 1024  # power_any_core.h any_plane_ok: even sizes up to kAnySlots x 2 kAnySlots (and the half-spectrum within LDS)
FAMILY_NAMES = ("small", "all", "bucket")
PLAN_FIELDS = ("family", "hn1", "hn2", "mn1", "mn2", "c2r_fuse", "threads", "fold_batches", "run_hn1", "run_hn2", "run_mn1", "run_mn2")


def plan(lib, H: int, W: int, family: int = -1):
    """sonar_power_any_plan as a dict, or None where the library refuses the size."""
    out = (C.c_int32 * len(PLAN_FIELDS))()
    if lib.sonar_power_any_plan(int(H), int(W), int(family), out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def _how(n: int, run: int):
    return "absent" if run == 2 else n if run == 1 else "direct1" if n == 1 else "direct"


def family_of(p, H: int, W: int) -> str:
    return f"bucket {H}x{W}" if p["family"] == 2 else FAMILY_NAMES[p["family"]]


def sites_of(p, H: int, W: int) -> frozenset:
    """The sites a plane size with plan ``p`` runs."""
    fam = family_of(p, H, W)
    return frozenset((
        (fam, "cols", 0, _how(p["hn1"], p["run_hn1"])),
        (fam, "cols", 1, _how(p["hn2"], p["run_hn2"])),
        (fam, "rows", 0, _how(p["mn1"], p["run_mn1"]), "fold" if p["c2r_fuse"] else "pre", p["fold_batches"]),
        (fam, "rows", 1, _how(p["mn2"], p["run_mn2"])),
        (fam, "threads", p["threads"]),
    ))


def pass_kinds(p) -> str:
    """'cols + rows' of a plan, each one of codelet/codelet, codelet/direct, direct/codelet, direct/direct, single codelet, single direct."""
    def axis(r1, r2):
        names = ("direct", "codelet")
        return f"single {names[r1]}" if r2 == 2 else f"{names[r1]}/{names[r2]}"

    return f"{axis(p['run_hn1'], p['run_hn2'])} + {axis(p['run_mn1'], p['run_mn2'])}"


def accepted_sizes(lib):
    """Every plane size the general-size kernels take (sonar_power_plane_kind == 2), ascending by area."""
    sizes = [(H, W) for H in range(2, H_MAX + 1, 2) for W in range(2, W_MAX + 1, 2) if lib.sonar_power_plane_kind(H, W) == 2]
    return sorted(sizes, key=lambda hw: (hw[0] * (hw[1] // 2 + 1), hw))


def domain_sites(lib):
    """{size: its sites} over the whole accepted domain."""
    return {hw: sites_of(plan(lib, *hw), *hw) for hw in accepted_sizes(lib)}


def greedy_cover(by_size, first=((2, 2),)):
    """A short list of small planes that reaches every site: after ``first``, always the size that reaches the most sites not reached
    yet, the smallest plane among equals."""
    picked = list(first)
    seen = set().union(*(by_size[hw] for hw in picked))
    every = set().union(*by_size.values())
    while seen != every:
        best = max(by_size, key=lambda hw: len(by_size[hw] - seen))  # (ascending by area: the first of the equals is the smallest)
        picked.append(best)
        seen |= by_size[best]
    return sorted(picked, key=lambda s: (s[0] * (s[1] // 2 + 1), s))


# greedy_cover over the 34,706 accepted sizes (214 sites); the eight SDXL buckets and 2 x 2 are among them
SWEEP = (
    (2, 2), (2, 6), (2, 8), (2, 18), (2, 20), (2, 26), (14, 22), (14, 24), (20, 36), (2, 392), (144, 4), (228, 2),
    (22, 40), (154, 4), (26, 36), (2, 578), (20, 68), (182, 6), (2, 828), (14, 124), (40, 44), (196, 8), (4, 618), (414, 4),
    (14, 186), (42, 70), (6, 548), (10, 328), (14, 236), (14, 248), (98, 40), (10, 410), (12, 352), (240, 18), (6, 822), (14, 354),
    (70, 72), (104, 48), (102, 50), (256, 20), (104, 56), (10, 656), (20, 328), (14, 472), (52, 128), (72, 98), (10, 738), (52, 144),
    (14, 590), (52, 160), (40, 210), (10, 902), (52, 176), (20, 492), (14, 708), (22, 456), (52, 192), (36, 288), (128, 84), (20, 574),
    (14, 826), (414, 26), (14, 828), (92, 128), (28, 450), (20, 656), (14, 944), (32, 442), (104, 144), (80, 192), (192, 80), (22, 722),
    (104, 152), (152, 104), (96, 168), (112, 144), (144, 112), (20, 820), (168, 96), (104, 160), (108, 162), (20, 902), (18, 1008), (18, 1010),
    (38, 484), (150, 128), (100, 200), (92, 234), (90, 280), (54, 512), (132, 264),
)


if __name__ == "__main__":
    import sonar_pkg

    _lib = sonar_pkg.load().hip_lib.load()
    _by_size = domain_sites(_lib)
    _cover = greedy_cover(_by_size)
    print(f"# {len(_by_size)} sizes, {len(set().union(*_by_size.values()))} sites, {len(_cover)} sizes cover them, "
          f"{sum(h * w for h, w in _cover)} elements")
    print("SWEEP = (")
    for i in range(0, len(_cover), 12):
        print("    " + " ".join(f"({h}, {w})," for h, w in _cover[i:i + 12]))
    print(")")
