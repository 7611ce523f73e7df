"""What the per-instance GEMM tests (test_gemm_fp8_instances_gpu.py, test_gemm_bf16_instances_gpu.py) share: strided views inside
sentinel-filled buffers, the float64 restatement of GELU-tanh and the bf16 ulp it is held to."""
import torch


def dev():
    return torch.device("cuda:0")


def _strided(rows, cols, ld, dtype, sentinel, r0=1, c0=16):
    """(buffer, view [rows, cols] at (r0, c0)) with the rest of the buffer holding `sentinel`."""
    buf = torch.full((rows + 2 * r0, ld), sentinel, dtype=dtype, device=dev())
    return buf, buf[r0:r0 + rows, c0:c0 + cols]


def _margins_untouched(buf, view_rows, view_cols, sentinel, r0=1, c0=16):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[r0:r0 + view_rows, c0:c0 + view_cols] = False
    return bool((buf[keep] == sentinel).all())


def _gelu64(y):
    """0.5 y (1 + tanh(u)) written as y / (1 + exp(-2u)): no cancellation for negative y (1 + tanh(u) is 0 in float64 below y = -7)."""
    return y / (1.0 + torch.exp(-1.5957691216057308 * (y + 0.044715 * y ** 3)))


def _bf16_ulp(x):
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def gelu_misses(got, y):
    """Mask of outputs `got` (bf16) more than 1 bf16 ulp from bf16(gelu64(y)), y float64 and exact.  Where |gelu(y)| < 2^-100, i.e.
    y < -10, the device's exp2 may overflow to a signed zero: there both sides must be below that.  A NaN output is a miss."""
    want = _gelu64(y).float().to(torch.bfloat16).double()
    got = got.double()
    tiny = want.abs() < 2.0 ** -100
    return ~((got - want).abs() <= _bf16_ulp(want)) & ~(tiny & (got.abs() < 2.0 ** -100))
