"""The generate-mode shuffle (csrc/shuffle.hip) restated on the host: Python integers on top of the Philox4x32-10 and
u01 statements of oracle/device_streams.py.  Nothing from the product.

  block(seed, stream, row, b)  Philox4x32-10 of counter (row lo, row hi | (stream hi << 16), b, stream lo) under the key
                               (seed lo, seed hi ^ DOMAIN) -- the distro blocks' layout, a domain of its own
  mask    row is shuffled when prob >= 1 or u01(word 0 of block(stream, row, 0)) < fp32(prob)
  offset  1 + ((word 0 of block(stream + 1, row, 0) >> 8) * (n - 1) >> 24): u01's 24 bits scaled to [1, n)
  key j   word j % 4 of block(stream + 2, row, j // 4) >> 8 (u01's 24 bits); value j moves to the rank of (key j, j)
"""
import numpy as np

from oracle import device_streams as ds

DOMAIN = 0x53484646
_M32, _M64 = 0xFFFFFFFF, 2**64 - 1


def blocks(seed: int, stream: int, row: int, count: int):
    """Blocks 0 .. count - 1 of (stream, row): [count][4] Python integers."""
    seed &= _M64
    c1 = ((row >> 32) | ((stream >> 32) << 16)) & _M32
    w = ds.philox4x32_10(np.full(count, row & _M32, dtype=np.uint64), np.full(count, c1, dtype=np.uint64), np.arange(count, dtype=np.uint64),
                         np.full(count, stream & _M32, dtype=np.uint64), seed & _M32, (seed >> 32) ^ DOMAIN)
    return [[int(w[q][b]) for q in range(4)] for b in range(count)]


def row_sources(seed: int, stream: int, row: int, n: int, prob: float, no_identity: bool):
    """perm with out[j] = in[perm[j]] for the row of global index ``row``."""
    shuffled = prob >= 1.0 or float(ds.u01(blocks(seed, stream, row, 1)[0][0])) < float(np.float32(prob))
    if not shuffled:
        return list(range(n))
    if no_identity:
        off = 1 + (((blocks(seed, stream + 1, row, 1)[0][0] >> 8) * (n - 1)) >> 24)
        assert 1 <= off < n
        return [(j + off) % n for j in range(n)]
    words = [w for b in blocks(seed, stream + 2, row, (n + 3) // 4) for w in b][:n]
    return [j for _key, j in sorted((w >> 8, j) for j, w in enumerate(words))]


def shuffled(x: np.ndarray, dim: int, prob: float, no_identity: bool, seed: int, stream: int, row_offset: int = 0) -> np.ndarray:
    """``x`` with every row along ``dim`` gathered through row_sources; rows are the row-major positions of the other dimensions."""
    dim %= x.ndim
    moved = np.moveaxis(x, dim, -1)
    rows2d = np.ascontiguousarray(moved).reshape(-1, x.shape[dim])
    out = np.empty_like(rows2d)
    for r in range(rows2d.shape[0]):
        out[r] = rows2d[r][row_sources(seed, stream, row_offset + r, x.shape[dim], prob, no_identity)]
    return np.ascontiguousarray(np.moveaxis(out.reshape(moved.shape), -1, dim))
