"""GPU: the e4m3-weight GEMM (flexam_gemm_w8 / flexam_gemm_w8_gate_residual, csrc/gemm.hip W8 instances) -- W is read as OCP e4m3
bytes and widened to bf16 in registers, so
  * every finite e4m3 code comes out exactly (one-hot A rows pick single W values into an fp32 output), NaN codes as NaN;
  * the result is BIT-identical to flexam_gemm_bf16 on W upcast to bf16, at every tile plan the bf16 GEMM can take (forced tile
    heights, the 192 x 192 tile on / off, tail split-K on / off) and with every epilogue, on strided A and row slices of a fused W;
  * argument errors are refused by the entry points before anything is launched."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, F8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float32
NAN_CODES = (0x7F, 0xFF)


def codes_matrix(n, k, dev):
    """W[n, k] = e4m3 code (n + k) % 256, NaN codes replaced by +0: every finite code (-0 and the subnormals included) in every K position."""
    c = (torch.arange(n, device=dev)[:, None] + torch.arange(k, device=dev)[None, :]) % 256
    for bad in NAN_CODES:
        c[c == bad] = 0
    return c.to(torch.uint8).view(F8)


def test_every_finite_e4m3_code_is_exact():
    from flexam_amd import hip
    dev = "cuda:0"
    M = K = 256
    for N in (256, 3072):
        w = codes_matrix(N, K, dev)
        for scale in (1.0, -2.0):
            a = (torch.eye(M, K, device=dev) * scale).to(BF)                   # row m picks K position m of every W row
            got = hip.gemm_w8(a, w, out_dtype=F32)
            want = a.float() @ w.float().T
            assert torch.equal(got, want), (N, scale)
            assert torch.equal(got[:, :256], scale * w.float()[:256].T)
    # all 256 codes, including both signs of every finite value, actually occur
    assert set(codes_matrix(256, 256, "cpu").view(torch.uint8).unique().tolist()) == set(range(256)) - set(NAN_CODES)
    # small integer A against the same codes, K = 64 ... 256 sums of exactly representable products
    g = torch.Generator(device=dev).manual_seed(5)
    a = torch.randint(-3, 4, (200, 64), device=dev, generator=g).to(BF)
    w = codes_matrix(512, 64, dev)
    w = torch.where((w.float().abs() >= 2.0 ** -2) & (w.float().abs() <= 16), w.float(), 0.0).to(F8)   # a range whose sums stay exact in fp32
    assert torch.equal(hip.gemm_w8(a, w, out_dtype=F32), a.float() @ w.float().T)


def test_nan_codes_come_out_as_nan():
    from flexam_amd import hip
    dev = "cuda:0"
    w = torch.zeros(256, 64, device=dev, dtype=torch.uint8)
    w[:, 0] = 0x38                                                            # 1.0
    w[3, 17] = 0x7F
    w[200, 40] = 0xFF
    a = torch.ones(64, 64, device=dev, dtype=BF)
    got = hip.gemm_w8(a, w.view(F8), out_dtype=F32)
    nan_cols = torch.isnan(got).all(0)
    assert nan_cols[3] and nan_cols[200] and int(nan_cols.sum()) == 2
    assert torch.equal(got[:, [0, 1, 255]], torch.ones(64, 3, device=dev))


def _cases():
    """(M, N, K) on ragged and DiT-like sizes; N multiples of 4 outside the 160-wide tile's widths."""
    return [(77, 200, 128), (300, 1000, 192), (1000, 3072, 3072), (2912, 3072, 3072), (2912, 6144, 3072), (700, 9216, 3072),
            (2912, 3072, 14336), (333, 14336, 3072)]


def _compare_all(dev="cuda:0", seed=0):
    """Every epilogue of every case: W8 against the bf16 GEMM on the upcast weights, bit for bit.  Returns the number of checks."""
    from flexam_amd import hip
    g = torch.Generator(device=dev).manual_seed(seed)
    n = 0
    for M, N, K in _cases():
        # A as a column slice of a wider buffer (row stride != K), W as a row slice of a fused e4m3 buffer
        abig = torch.randn(M, K + 128, device=dev, generator=g).to(BF)
        a = abig[:, 64:64 + K]
        wf = (torch.randn(N + 96, K, device=dev, generator=g) * 0.25).to(F8)
        w = wf[32:32 + N]
        wb = w.to(BF)
        bias = torch.randn(N, device=dev, generator=g)
        for epi, odt in ((hip.EPI_NONE, BF), (hip.EPI_GELU_TANH, BF), (hip.EPI_NONE, F32)):
            got = hip.gemm_w8(a, w, bias, epilogue=epi, out_dtype=odt)
            want = hip.gemm(a, wb, bias, epilogue=epi, out_dtype=odt)
            assert torch.equal(got.view(torch.int16 if odt == BF else torch.int32), want.view(torch.int16 if odt == BF else torch.int32)), \
                (M, N, K, epi, odt)
            n += 1
        # gated residual with a per-row gate index table, and without a gate
        x0 = torch.randn(M, N, device=dev, generator=g)
        gate = torch.randn(5, N, device=dev, generator=g)
        grow = torch.randint(0, 5, (M,), device=dev, generator=g, dtype=torch.int32)
        for kw in (dict(gate=gate, gate_row=grow), dict()):
            xa, xb = x0.clone(), x0.clone()
            hip.gemm_w8_gate_residual(a, w, bias, xa, **kw)
            hip.gemm_gate_residual(a, wb, bias, xb, **kw)
            assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), (M, N, K, "gate-residual", bool(kw))
            n += 1
        # hip.gemm / gemm_gate_residual route an e4m3 weight to the W8 kernel themselves
        assert torch.equal(hip.gemm(a, w, bias).view(torch.int16), hip.gemm(a, wb, bias).view(torch.int16))
    return n


@pytest.mark.parametrize("mt", ["", "4", "5", "6", "7", "8"])
@pytest.mark.parametrize("n192", ["0", "2"])
def test_bit_identical_to_bf16_gemm_on_upcast_weights(monkeypatch, mt, n192):
    """FLEXAM_GEMM_MT (forced tile height; "" = the planner's choice) and FLEXAM_GEMM_N192 (0: 256-wide tiles only, 2: the 192 x 192
    tile wherever N % 192 == 0) steer both kernels the same way; split-K stays at its default (on) here."""
    if mt:
        monkeypatch.setenv("FLEXAM_GEMM_MT", mt)
    else:
        monkeypatch.delenv("FLEXAM_GEMM_MT", raising=False)
    monkeypatch.setenv("FLEXAM_GEMM_N192", n192)
    assert _compare_all(seed=int(mt or 0) * 3 + int(n192)) == len(_cases()) * 5


def test_bit_identical_with_split_k_off():
    """FLEXAM_GEMM_SPLITK is read once per process: a fresh interpreter with the tail split-K off, planner's and forced tile plans."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, os; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gemm_w8_gpu as T\n"
            "for mt in ('', '4', '8'):\n"
            "    os.environ['FLEXAM_GEMM_MT'] = mt\n"
            "    print(T._compare_all(seed=11))\n") % (root, os.path.join(root, "tests"))
    env = dict(os.environ, FLEXAM_GEMM_SPLITK="0")
    env.pop("FLEXAM_GEMM_MT", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split() == [str(len(_cases()) * 5)] * 3


def test_argument_errors_are_refused_before_launch():
    import ctypes
    from flexam_amd import hip
    lib = hip.lib()
    dev = "cuda:0"
    a = torch.zeros(64, 128, device=dev, dtype=BF)
    w = torch.zeros(256, 128, device=dev, dtype=F8)
    c = torch.zeros(64, 256, device=dev, dtype=BF)
    x = torch.zeros(64, 256, device=dev, dtype=F32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def gemm(**kw):
        args = dict(A=P(a), lda=128, W=P(w), ldw=128, bias=None, C=P(c), ldc=256, M=64, N=256, K=128, epi=0, f32=0, koff=None, ws=None,
                    wsb=0, stream=None)
        args.update(kw)
        rc = lib.flexam_gemm_w8(*args.values())
        return rc, lib.flexam_last_error().decode()

    def gres(**kw):
        args = dict(A=P(a), lda=128, W=P(w), ldw=128, bias=None, X=P(x), ldx=256, gate=None, gate_ld=0, gate_row=None, rpb=0, M=64, N=256,
                    K=128, koff=None, ws=None, wsb=0, stream=None)
        args.update(kw)
        rc = lib.flexam_gemm_w8_gate_residual(*args.values())
        return rc, lib.flexam_last_error().decode()

    torch.cuda.synchronize()
    c.fill_(7.0)
    for kw, msg in ((dict(A=None), "null pointer"), (dict(W=None), "null pointer"), (dict(C=None), "null pointer"),
                    (dict(K=96), "multiple of 64"), (dict(ldw=120), "16-byte rows"), (dict(W=ctypes.c_void_p(w.data_ptr() + 8)), "aligned"),
                    (dict(epi=7), "unknown epilogue"), (dict(epi=1, f32=1), "f32 output"), (dict(N=160), "160-wide")):
        rc, err = gemm(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    for kw, msg in ((dict(X=None), "null pointer"), (dict(K=100), "K%64"), (dict(ldw=136), "16-byte rows"),
                    (dict(gate=P(x), gate_ld=256), "gate needs gate_row")):
        rc, err = gres(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()) and bool((x == 0).all())                   # nothing ran
    # the Python wrappers raise
    with pytest.raises(RuntimeError):
        hip.gemm_w8(a, w[:, :96].contiguous())
    with pytest.raises(RuntimeError):
        hip.gemm_w8(a, w.to(BF))
    with pytest.raises(RuntimeError):
        hip.gemm_w8(a, torch.zeros(160, 128, device=dev, dtype=F8))
