"""CPU: the numpy restatement of checksum_kernel (tests/checksum_restatement.py) that test_dit_row_kernels_gpu.py holds the kernel to
bit for bit -- checked here against the published splitmix64 sequence and against a plain Python-integer restatement, and for the
sensitivities the fingerprint is relied on for (a changed bit, two swapped words, an extra zero byte)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import checksum_restatement as R  # noqa: E402

M64 = (1 << 64) - 1


def mix_int(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def checksum_int(data: bytes):
    """The same sums with Python integers, one word at a time, in the kernel's own order of terms."""
    nw = len(data) // 4
    s0 = s1 = 0
    for i in range(nw):
        x = (int.from_bytes(data[4 * i:4 * i + 4], "little") + (i + 1) * 0x9E3779B97F4A7C15) & M64
        s0, s1 = (s0 + mix_int(x)) & M64, (s1 + mix_int(x ^ 0xD6E8FEB86659FD93)) & M64
    for j, t in enumerate(data[4 * nw:]):
        x = (t + (nw + 1 + j) * 0x9E3779B97F4A7C15) & M64
        s0, s1 = (s0 + mix_int(x)) & M64, (s1 + mix_int(x ^ 0xD6E8FEB86659FD93)) & M64
    s0 = (s0 + mix_int(len(data))) & M64
    return tuple(v - (1 << 64) if v >> 63 else v for v in (s0, s1))


def test_mix_is_splitmix64():
    """splitmix64 seeded with 0 yields mix(G), mix(2G), mix(3G): 0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f."""
    got = R.mix(np.arange(1, 4, dtype=np.uint64) * R.G)
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert int(R.mix(np.array([0], dtype=np.uint64))[0]) == 0


def test_restatement_matches_python_integers_at_every_tail_length():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 5, 7, 8, 63, 257, 1027):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert R.checksum(data) == checksum_int(data), n
    assert R.checksum(bytes(4))[0] == checksum_int(bytes(4))[0]


def test_restatement_sensitivities():
    rng = np.random.default_rng(6)
    data = bytearray(rng.integers(0, 256, 4099, dtype=np.uint8).tobytes())
    base = R.checksum(bytes(data))
    for bit in rng.choice(len(data) * 8, 64, replace=False):
        d = bytearray(data)
        d[bit // 8] ^= 1 << (bit % 8)
        assert R.checksum(bytes(d)) != base
    d = bytearray(data)
    d[0:4], d[40:44] = data[40:44], data[0:4]
    assert data[0:4] != data[40:44] and R.checksum(bytes(d)) != base
    assert R.checksum(bytes(data) + b"\0") != base
    assert R.checksum(bytes(4)) != R.checksum(bytes(5)) != R.checksum(bytes(8))
