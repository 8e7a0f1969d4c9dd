#!/usr/bin/env python3
"""Kernel resources of the BUILT library, read from its code objects' metadata in seconds (no recompilation):

    python tools/so_kernels.py [libsonar_hip.so] [--scratch]      (--scratch: only the kernels with a private segment)
    python tools/so_kernels.py [libsonar_hip.so] --digest         (sha256 of every device function's machine code, sorted by name)

The .hip_fatbin section of the shared object holds one clang offload bundle per translation unit; each is unbundled for gfx950 and its
amdhsa.kernels notes are read with llvm-readelf.  `kernels(path)` returns [{name, vgpr, sgpr, lds, scratch, spill_v, spill_s}].

--digest is for refactors that must leave the device code alone: two builds with equal listings run the same instructions with the same
resources.  Per function symbol of every code object: sha256 of its bytes in .text; per kernel also sha256 of its 64-byte descriptor
(<name>.kd) and the metadata fields above.  `digests(path)` returns the lines."""
import contextlib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _readelf(*args):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), *args], capture_output=True, text=True, check=True).stdout


def _sections(path):
    """{index: (name, address, file offset, size)}"""
    secs = {}
    for line in _readelf("-S", "-W", path).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S*)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16))
    return secs


def _section(path, name=".hip_fatbin"):
    for sname, _, off, size in _sections(path).values():
        if sname == name:
            with open(path, "rb") as fh:
                fh.seek(off)
                return fh.read(size)
    raise RuntimeError(f"{path}: no {name} section")


@contextlib.contextmanager
def _code_objects(path=None):
    """The gfx950 code object of every translation unit of the library, as files in a temporary directory."""
    path = path or os.path.join(ROOT, "comfyui-sonar_amd", "libsonar_hip.so")
    blob = _section(path)
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    with tempfile.TemporaryDirectory() as tmp:
        cos = []
        for i, s in enumerate(starts):
            e = starts[i + 1] if i + 1 < len(starts) else len(blob)
            bundle = os.path.join(tmp, f"b{i}.bundle")
            with open(bundle, "wb") as fh:
                fh.write(blob[s:e])
            co = os.path.join(tmp, f"b{i}.co")
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={bundle}", f"--output={co}"], capture_output=True, text=True)
            if os.path.exists(co) and os.path.getsize(co) > 0:
                cos.append(co)
        yield cos


def _metadata(co):
    rows = []
    for block in _readelf("--notes", co).split("  - .agpr_count:")[1:]:
        def field(key, default="0"):
            m = re.search(r"\." + key + r":\s+(\S+)", block)
            return m.group(1) if m else default
        rows.append({"name": field("name", "?"), "vgpr": int(field("vgpr_count")), "sgpr": int(field("sgpr_count")),
                     "lds": int(field("group_segment_fixed_size")), "scratch": int(field("private_segment_fixed_size")),
                     "spill_v": int(field("vgpr_spill_count")), "spill_s": int(field("sgpr_spill_count"))})
    return rows


def kernels(path=None):
    with _code_objects(path) as cos:
        rows = [r for co in cos for r in _metadata(co)]
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    for r, n in zip(rows, names):
        r["pretty"] = re.sub(r"\(.*", "", n)
    return rows


def digests(path=None):
    """One line per function symbol (and per kernel descriptor and kernel metadata record) of every code object, sorted by name."""
    lines = []
    with _code_objects(path) as cos:
        for co in cos:
            secs = _sections(co)
            with open(co, "rb") as fh:
                image = fh.read()
            symbols = {}  # name -> (type, bytes)
            for line in _readelf("-s", "-W", co).splitlines():
                f = line.split()
                if len(f) == 8 and f[0].endswith(":") and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
                    _, addr, off, _ = secs[int(f[6])]
                    start = off + int(f[1], 16) - addr
                    symbols[f[7]] = (f[3], image[start:start + int(f[2], 0)])
            for name, (kind, data) in symbols.items():
                if kind == "FUNC":
                    lines.append(f"{hashlib.sha256(data).hexdigest()}  {name}")
            for r in _metadata(co):
                kind, data = symbols[r["name"] + ".kd"]
                assert kind == "OBJECT" and len(data) == 64, r["name"]
                lines.append(f"{hashlib.sha256(data).hexdigest()}  {r['name']}.kd")
                lines.append(f"vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']} spill_v {r['spill_v']} spill_s {r['spill_s']}  {r['name']}.meta")
    return sorted(lines, key=lambda l: (l.rsplit("  ", 1)[1], l))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--digest" in sys.argv:
        print("\n".join(digests(args[0] if args else None)))
        return
    rows = kernels(args[0] if args else None)
    only = "--scratch" in sys.argv
    shown = [r for r in rows if r["scratch"] > 0] if only else rows
    for r in sorted(shown, key=lambda r: r["pretty"]):
        print(f"vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']:4d} (spilled vector {r['spill_v']:3d}, scalar {r['spill_s']:3d})  {r['pretty']}")
    print(f"{len(rows)} kernels, {sum(1 for r in rows if r['scratch'] > 0)} with a scratch segment, {sum(1 for r in rows if r['vgpr'] > 128)} above 128 vector registers")


if __name__ == "__main__":
    main()
