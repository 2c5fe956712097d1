"""Host restatements of the device draws (csrc/rng.hip: krrn_randperm_i32, krrn_randperm_multi_i32,
krrn_ransac_subsets, krrn_rng_advance) and of the radix-selected `choose` subset of csrc/inputs.hip
(krrn_choose_points), written from include/krrn_hip.h and the kernels' comments in numpy.uint64 (whose
arithmetic wraps modulo 2^64 as the device's unsigned long long does). Every one of those kernels is integer
exact, so a GPU test compares with array_equal, never with a tolerance. Nothing here imports the package.

A seed is the int64 tensor's bits read as unsigned (-1 is 2^64 - 1); krrn_rng_advance adds one modulo 2^64.
"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
STREAM_MUL = 0xD1B54A32D192ED03
ROW_MUL = 0x632BE59BD9B4E019
CHOOSE_STREAM_MAX = 65534  # krrn_choose_points: 0 <= stream_id <= 65534 (the id enters the key's top 16 bits)

_U = np.uint64


def u64(seed: int) -> int:
    """The bits of an int64 (or already unsigned) seed as an unsigned 64-bit integer."""
    return int(seed) & M64


def advance(seed: int, steps: int = 1) -> int:
    """krrn_rng_advance `steps` times: seed + steps modulo 2^64, returned as the int64 the tensor then holds."""
    v = (u64(seed) + steps) & M64
    return v - (1 << 64) if v >> 63 else v


def mix64(z):
    """splitmix64's step (add the golden gamma, then the finaliser). A Python int gives a Python int; an
    array of uint64 is mixed element-wise."""
    if isinstance(z, np.ndarray):
        with np.errstate(over="ignore"):
            z = z.astype(_U) + _U(GOLDEN)
            z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
            return z ^ (z >> _U(31))
    z = (int(z) + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _row_base(seed: int, stream: int, row: int) -> int:
    # stream + 1 and row + 1 are unsigned 32-bit sums on the device: stream 2^32 - 1 gives a factor of 0
    a = mix64(u64(seed) ^ ((STREAM_MUL * ((int(stream) + 1) & 0xFFFFFFFF)) & M64))
    return mix64((a + ROW_MUL * ((int(row) + 1) & 0xFFFFFFFF)) & M64)


def rand32(seed: int, stream: int, row: int, i):
    """The generator's 32-bit value number `i` (an int, or an array of counters) of (seed, stream, row)."""
    b = _row_base(seed, stream, row)
    if isinstance(i, np.ndarray):
        with np.errstate(over="ignore"):
            return (mix64(_U(b) + i.astype(_U)) >> _U(32)).astype(np.uint32)
    return mix64((b + int(i)) & M64) >> 32


def randperm(seed: int, stream: int, row: int, n: int, k: int) -> np.ndarray:
    """Row `row` of krrn_randperm_i32: the indices 0..n-1 sorted by (rand32, index), the first k. int32 [k]."""
    key = rand32(seed, stream, row, np.arange(n, dtype=_U)).astype(_U) << _U(32) | np.arange(n, dtype=_U)
    return (np.sort(key)[:k] & _U(0xFFFFFFFF)).astype(np.int32)


def randperm_rows(seed: int, stream: int, n: int, k: int, rows: int) -> np.ndarray:
    return np.stack([randperm(seed, stream, r, n, k) for r in range(rows)])


def ransac_subsets(seed: int, stream: int, B: int, H: int, P: int) -> np.ndarray:
    """krrn_ransac_subsets: for hypothesis e = b*H + h (the generator's row) five distinct indices in [0, P),
    each (rand32 * P) >> 32 of a counter that runs on through the rejected duplicates; a draw is kept
    regardless once the counter has passed 4096. int32 [B][H][5]."""
    out = np.zeros((B * H, 5), np.int32)
    for e in range(B * H):
        vals = (rand32(seed, stream, e, np.arange(64, dtype=_U)).astype(_U) * _U(P)) >> _U(32)
        ids, ctr = [], 0
        for _ in range(5):
            while True:
                if ctr >= len(vals):
                    more = np.arange(len(vals), 2 * len(vals), dtype=_U)
                    vals = np.concatenate([vals, (rand32(seed, stream, e, more).astype(_U) * _U(P)) >> _U(32)])
                x = int(vals[ctr])
                ctr += 1
                if x not in ids or ctr > 4096:
                    ids.append(x)
                    break
        out[e] = ids
    return out.reshape(B, H, 5)


def choose_base(seed: int, stream_id: int, crop: int) -> int:
    """The key base of crop `crop`: (seed * golden) ^ ((stream_id + 1) << 48) ^ (crop << 24), modulo 2^64."""
    if not 0 <= stream_id <= CHOOSE_STREAM_MAX:
        raise ValueError(f"stream_id {stream_id} outside 0..{CHOOSE_STREAM_MAX}")
    return ((u64(seed) * GOLDEN) & M64) ^ (((stream_id + 1) << 48) & M64) ^ ((crop << 24) & M64)


def mix32(x):
    """The high half of mix64."""
    if isinstance(x, np.ndarray):
        return (mix64(x) >> _U(32)).astype(np.uint32)
    return mix64(x) >> 32


def choose_keys(seed: int, stream_id: int, crop: int, count: int) -> np.ndarray:
    """The 32-bit key of each rank 0..count-1 (rank = position among the crop's mask pixels, row-major)."""
    with np.errstate(over="ignore"):
        return mix32(_U(choose_base(seed, stream_id, crop)) + np.arange(count, dtype=_U))


def choose_subset(seed: int, stream_id: int, crop: int, count: int, N: int) -> np.ndarray:
    """The ranks of the N smallest (key, rank) pairs among `count`, ascending. int64 [N]."""
    assert count > N >= 1
    pair = choose_keys(seed, stream_id, crop, count).astype(_U) << _U(32) | np.arange(count, dtype=_U)
    return np.sort((np.sort(pair)[:N] & _U(0xFFFFFFFF)).astype(np.int64))


def choose(mask, N: int, seed: int = 0, stream_id: int = 0, crop: int = 0) -> np.ndarray:
    """krrn_choose_points' `choose` of one crop: the mask pixels (crop-local r*S + c) in row-major order,
    the radix-selected subset when there are more than N, wrap-padded when fewer, zeros when none."""
    cand = np.asarray(mask).reshape(-1).nonzero()[0].astype(np.int64)
    count = len(cand)
    if count == 0:
        return np.zeros(N, np.int64)
    if count > N:
        return cand[choose_subset(seed, stream_id, crop, count, N)]
    return np.pad(cand, (0, N - count), "wrap")
