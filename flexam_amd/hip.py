"""ctypes binding of libflexam_hip.so (C ABI in include/flexam_hip.h) + thin tensor wrappers.

PyTorch is plumbing here: it owns device memory and the stream; every function below passes raw
device pointers, sizes and strides to the HIP library and raises RuntimeError on a non-zero
return code.  There is NO fallback: if the shared library is missing, or a tensor is not on a
GPU, the call fails loudly (a silent CPU/eager path would void every parity claim).
"""
import ctypes
import os
from collections import namedtuple
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libflexam_hip.so")

_P, _I, _L, _F = c_void_p, c_int, c_int64, c_float
_SIGNATURES = abi.signatures(abi.PROTOTYPES)        # {name: (argtypes, restype)} of include/flexam_hip.h, in header order
_STREAM_ORDERED = frozenset(n for n, _ in abi.stream_ordered(abi.PROTOTYPES))
_REPLAYABLE = frozenset(n for n, _ in abi.replayable(abi.PROTOTYPES))
EPI_NONE, EPI_GELU_TANH = abi.CONSTANTS["FLEXAM_EPI_NONE"], abi.CONSTANTS["FLEXAM_EPI_GELU_TANH"]

_lib = None


def load_library(path: str = None) -> ctypes.CDLL:
    """Loads libflexam_hip.so and declares every entry point.  No compute call is made, so this
    also works on a host without a GPU (used by the CPU test that checks the exported symbols)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m flexam_amd.build` "
                           "(flexam_amd has no CPU or eager fallback)")
    lib = ctypes.CDLL(path)
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def lib():
    """The library -- or, while a command list is being recorded (`record()`), the recorder in front of it."""
    if _rec is not None:
        return _rec
    return _lib if _lib is not None else load_library()


# ----------------------------------------------------------------------------- command lists (csrc/replay.hip)
REPLAY_MAX_ARGS = abi.CONSTANTS["FLEXAM_REPLAY_MAX_ARGS"]


class _Arg(ctypes.Union):
    _fields_ = [("i", c_int64), ("f", ctypes.c_double), ("p", c_void_p)]


class _Cmd(ctypes.Structure):
    _fields_ = [("fn", ctypes.c_int32), ("nargs", ctypes.c_int32), ("a", _Arg * REPLAY_MAX_ARGS)]


# entry points that read HOST arrays during the call (flexam_hip.h): a recorded pointer to a temporary host array would dangle
_NOT_RECORDABLE = ("flexam_lincomb_f32",)
_rec = None              # the active _Recorder (one at a time, per process: recording happens on the thread that drives the engine)
_FN_IDS = {}


def _fn_id(name: str) -> int:
    if name not in _FN_IDS:
        real = _lib if _lib is not None else load_library()
        _FN_IDS[name] = int(real.flexam_fn_id(name.encode()))
    return _FN_IDS[name]


class Plan:
    """A recorded stretch of the engine's work: C segments (arrays of flexam_cmd, each re-issued by ONE flexam_replay call) interleaved
    with host operations (Python callables: collectives, waits, torch copies -- whatever the engine wrapped in `host_op`).  `keep` holds
    every tensor whose pointer sits in a command, so no recorded address can be handed to anybody else while the plan lives."""

    def __init__(self):
        self.items, self.keep, self.launches = [], [], 0

    def run(self):
        real = _lib if _lib is not None else load_library()
        st = _stream()
        failed = c_int64(-1)
        for kind, a, b in self.items:
            if kind == "c":
                rc = real.flexam_replay(a, b, ctypes.byref(failed), st)
                if rc != 0:
                    name = real.flexam_fn_name(a[failed.value].fn) if failed.value >= 0 else b"?"
                    raise RuntimeError(f"flexam_replay: command {failed.value} ({(name or b'?').decode()}) failed with code {rc}: "
                                       f"{real.flexam_last_error().decode()}")
            else:
                a()


class _Recorder:
    """Stands in for the library while a plan is recorded: every stream-ordered entry point is CALLED (the recording step is a real
    step) and appended to the open C segment as (function id, argument words); anything else (queries, flexam_last_error) passes
    through.  The stream argument is not recorded: a replay runs on the stream it is issued on."""

    def __init__(self, plan: Plan):
        self.plan, self.seg = plan, []
        self._wrapped = {}

    def __getattr__(self, name):
        real = _lib if _lib is not None else load_library()
        fn = getattr(real, name)
        if name not in _REPLAYABLE:
            return fn
        if name in _NOT_RECORDABLE:
            raise RuntimeError(f"{name} takes host arrays and cannot be part of a recorded launch plan")
        w = self._wrapped.get(name)
        if w is None:
            kinds = _SIGNATURES[name][0][:-1]

            def w(*args, _fn=fn, _fid=_fn_id(name), _kinds=kinds, _name=name):
                rc = _fn(*args)
                if rc == 0:
                    if len(args) != len(_kinds) + 1:
                        raise RuntimeError(f"{_name}: {len(args)} arguments recorded, the signature has {len(_kinds) + 1}")
                    self.seg.append((_fid, _kinds, args[:-1]))
                return rc
            self._wrapped[name] = w
        return w

    def flush(self):
        if not self.seg:
            return
        arr = (_Cmd * len(self.seg))()
        for c, (fid, kinds, args) in zip(arr, self.seg):
            c.fn, c.nargs = fid, len(args)
            for j, (k, v) in enumerate(zip(kinds, args)):
                if k is _P:
                    c.a[j].p = v
                elif k is _F:
                    c.a[j].f = float(v)
                else:
                    c.a[j].i = int(v)
        self.plan.items.append(("c", arr, len(self.seg)))
        self.plan.launches += len(self.seg)
        self.seg = []


class record:
    """`with hip.record() as plan:` -- everything the block of code launches through this module is executed AND recorded into `plan`
    (Plan.run() re-issues it).  Valid for code whose launches depend only on things that do not change between runs: buffer addresses,
    shapes, scalars (the caller's business: DiTEngine keys its plans on all of them).  Host-side work in between goes through
    `host_op`."""

    def __init__(self):
        self.plan = Plan()

    def __enter__(self):
        global _rec
        if _rec is not None:
            raise RuntimeError("flexam_amd.hip.record: already recording")
        _rec = _Recorder(self.plan)
        return self.plan

    def __exit__(self, et, ev, tb):
        global _rec
        rec, _rec = _rec, None
        if et is None:
            rec.flush()
        return False


def host_op(fn):
    """Runs `fn()` now; while a plan is recorded it also closes the open C segment and becomes a host step of the plan (run again, in
    this place, by every Plan.run()).  For what is not a call into the library: collectives, Work.wait(), torch copies.  A host step is
    opaque: library calls it makes itself (an emulated collective's delay kernel on its side stream) are part of the step, not of a C
    segment -- recording is suspended while it runs."""
    global _rec
    if _rec is None:
        return fn()
    rec = _rec
    rec.flush()
    rec.plan.items.append(("py", fn, None))
    _rec = None
    try:
        return fn()
    finally:
        _rec = rec


def delay_us(us: float):
    """Emulation aid: the current stream waits `us` microseconds (flexam_delay_us)."""
    _call("flexam_delay_us", float(us))


def recording() -> bool:
    return _rec is not None


def _call(name: str, *args, stream=None):
    """Calls entry point `name` through lib() (so a recorder stands in front of it); stream-ordered ones get the current stream (or
    `stream`, where the caller already asked for it) as their last argument.  A non-zero return code raises."""
    if name in _STREAM_ORDERED:
        args += (_stream() if stream is None else stream,)
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}: {lib().flexam_last_error().decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("flexam_amd.hip: tensor is not on a GPU (there is no CPU path)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"flexam_amd.hip: expected {dtype}, got {t.dtype}")
    if _rec is not None:
        _rec.plan.keep.append(t)                   # a recorded address stays this tensor's for as long as the plan lives
    return t.data_ptr()


def _raw(t):
    """data_ptr() of scratch the wrappers pass without a dtype check (workspaces, byte images); kept alive by a plan being recorded."""
    if _rec is not None:
        _rec.plan.keep.append(t)
    return t.data_ptr()


def _rows(t):
    """2-D view requirements: last dim contiguous; returns (rows, cols, row_stride)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError(f"flexam_amd.hip: expected a 2-D row-major view, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


BF16, F32, I32, I64, U8, F8 = torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8, torch.float8_e4m3fn


def device_check():
    _call("flexam_device_check")


def set_cu_budget(cus: int = 0):
    """Plan the library's persistent grids for `cus` CUs of the current device (0 = all); see flexam_set_cu_budget."""
    _call("flexam_set_cu_budget", int(cus))


def num_cus() -> int:
    """Compute units the library plans its grids for on the current device (flexam_device_cus: 256 on MI355X)."""
    return int(lib().flexam_device_cus())


# ----------------------------------------------------------------------------- GEMM
_GEMM_WS = {}
GEMM_WS_BYTES = abi.CONSTANTS["FLEXAM_GEMM_WS_BYTES"]
WS_CACHE_SLOTS = 8                                  # (device, stream) pairs that keep their scratch; older ones are dropped


def _ws_slot(cache: dict, key, make):
    """Scratch per (device, stream) -- launches that can run concurrently never share it -- in a small LRU: a program that
    creates streams per call does not grow memory without bound.  Dropping an entry waits for its device first (rare: the
    9th distinct stream), so no kernel still writes the slabs when the allocator hands them out again."""
    hit = cache.pop(key, None)
    if hit is None:
        while len(cache) >= WS_CACHE_SLOTS:
            old = next(iter(cache))
            torch.cuda.synchronize(old[0])
            del cache[old]
        hit = make()
    cache[key] = hit                                # re-inserted last = most recently used
    return hit


def _ws_key(device, stream: int):
    return (device.index if device.index is not None else torch.cuda.current_device(), stream)


def _gemm_workspace(device, stream: int):
    """Tail split-K scratch (64 MiB of partial-sum slabs) handed to every GEMM call, per (device, stream)."""
    return _ws_slot(_GEMM_WS, _ws_key(device, stream), lambda: torch.empty(GEMM_WS_BYTES, device=device, dtype=torch.uint8))


def gemm(a, w, bias=None, out=None, epilogue=EPI_NONE, out_dtype=BF16, a_koff=None, m=None, k=None):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias).  a bf16, w bf16 or float8_e4m3fn (qfloat8 weight storage, read as such by
    flexam_gemm_w8: no bf16 copy of w, bit-identical to the GEMM on w.to(bfloat16)); 2-D views, row stride free.
    With a_koff (int64 [K/64]) `a` is only a base view: rows are `m`, K = `k` (implicit conv)."""
    who, wdt = ("gemm_w8", F8) if w.dtype == F8 else ("gemm", BF16)
    am, ak, lda = _rows(a)
    wn, wk, ldw = _rows(w)
    M = am if m is None else m
    K = wk if k is None else k
    if a_koff is None and ak != K:
        raise RuntimeError(f"{who}: K mismatch a {ak} vs w {K}")
    if out is None:
        out = torch.empty(M, wn, device=a.device, dtype=out_dtype)
    om, on, ldc = _rows(out)
    if (om, on) != (M, wn):
        raise RuntimeError(f"{who}: out shape {tuple(out.shape)} != ({M}, {wn})")
    st = _stream()
    ws = _gemm_workspace(a.device, st)
    _call("flexam_gemm_w8" if wdt == F8 else "flexam_gemm_bf16", _ptr(a, BF16), lda, _ptr(w, wdt), ldw, _ptr(bias, F32), _ptr(out), ldc, M,
          wn, K, epilogue, 1 if out.dtype == F32 else 0, _ptr(a_koff, I64), _raw(ws), ws.numel(), stream=st)
    return out


def gemm_gate_residual(a, w, bias, x, gate=None, gate_row=None, rows_per_batch=0, a_koff=None):
    """x[M,N] (fp32, in place) += bf16(a @ w^T + bias) * gate[row]; w bf16 or float8_e4m3fn as in gemm.  With a_koff `a` is a base
    view (implicit conv) and M, K come from x and w."""
    who, wdt = ("gemm_w8_gate_residual", F8) if w.dtype == F8 else ("gemm_gate_residual", BF16)
    am, ak, lda = _rows(a)
    N, K, ldw = _rows(w)
    M, xn, ldx = _rows(x)
    if (a_koff is None and (ak != K or am != M)) or xn != N:
        raise RuntimeError(f"{who}: shape mismatch")
    gate_ld = gate.stride(0) if gate is not None else 0
    st = _stream()
    ws = _gemm_workspace(a.device, st)
    _call("flexam_gemm_w8_gate_residual" if wdt == F8 else "flexam_gemm_bf16_gate_residual", _ptr(a, BF16), lda, _ptr(w, wdt), ldw,
          _ptr(bias, F32), _ptr(x, F32), ldx, _ptr(gate, F32), gate_ld, _ptr(gate_row, I32), rows_per_batch, M, N, K, _ptr(a_koff, I64),
          _raw(ws), ws.numel(), stream=st)
    return x


# ----------------------------------------------------------------------------- e4m3 weights, bf16 activations (qfloat8 modes)
def _e4m3(w):
    if w.dtype not in (F8, U8):
        raise RuntimeError(f"flexam_amd.hip: expected float8_e4m3fn (or uint8 e4m3 bytes) weights, got {w.dtype}")
    return w.view(F8)


def gemm_w8_takes(n: int) -> bool:
    """Whether flexam_gemm_w8* has a plan for output width `n`: every width except those the bf16 GEMM runs on its 160-wide tile
    (csrc/gemm.hip launch(): N <= 160, and multiples of 160 that are not of 256 up to 480 -- all of them with FLEXAM_GEMM_N160=2;
    none with FLEXAM_GEMM_N160=0), which has no e4m3 form."""
    mode = int(os.environ.get("FLEXAM_GEMM_N160", "1") or 0)
    narrow = n <= 160
    mult160 = n % 160 == 0 and n % 256 != 0 and (n <= 480 or mode == 2)
    return not (mode and (narrow or mult160))


def gemm_w8(a, w, bias=None, out=None, epilogue=EPI_NONE, out_dtype=BF16, a_koff=None, m=None, k=None):
    """gemm() for w [N, K] OCP e4m3 only: float8_e4m3fn, or the same bytes as uint8 (a row slice of a fused buffer is fine)."""
    return gemm(a, _e4m3(w), bias, out, epilogue, out_dtype, a_koff, m, k)


def gemm_w8_gate_residual(a, w, bias, x, gate=None, gate_row=None, rows_per_batch=0, a_koff=None):
    """gemm_gate_residual() for w [N, K] OCP e4m3 only (float8_e4m3fn or uint8 bytes)."""
    return gemm_gate_residual(a, _e4m3(w), bias, x, gate, gate_row, rows_per_batch, a_koff)


# ----------------------------------------------------------------------------- fp8 GEMM (BASELINE configs[4])
def quantize_rows_fp8(x, q=None, scale=None):
    """x [M, K] bf16 rows -> (q [M, K] uint8 holding OCP e4m3 bytes, scale [M] fp32) with x ~ q * scale[:, None]."""
    M, K, ldx = _rows(x)
    if q is None:
        q = torch.empty(M, K, device=x.device, dtype=U8)
    if scale is None:
        scale = torch.empty(M, device=x.device, dtype=F32)
    _call("flexam_quantize_rows_fp8", _ptr(x, BF16), ldx, _ptr(q, U8), q.stride(0), _ptr(scale, F32), M, K)
    return q, scale


def gemm_fp8(a8, a_scale, w8, w_scale, bias=None, out=None, epilogue=EPI_NONE):
    """out[M,N] bf16 = epi((a8 @ w8^T) * a_scale[:, None] * w_scale[None, :] + bias); a8 [M,K], w8 [N,K] e4m3 bytes."""
    M, K, lda = _rows(a8)
    N, wk, ldw = _rows(w8)
    if wk != K:
        raise RuntimeError(f"gemm_fp8: K mismatch a {K} vs w {wk}")
    if out is None:
        out = torch.empty(M, N, device=a8.device, dtype=BF16)
    _call("flexam_gemm_fp8", _ptr(a8, U8), lda, _ptr(a_scale, F32), _ptr(w8, U8), ldw, _ptr(w_scale, F32), _ptr(bias, F32), _ptr(out, BF16),
          out.stride(0), M, N, K, epilogue)
    return out


def gemm_fp8_gelu_q(a8, a_scale, w8, w_scale, bias, out_scale, q_out):
    """q_out[M,N] (e4m3 bytes) = e4m3(gelu_tanh((a8 @ w8^T) * scales + bias) / out_scale[:, None]): FFN1 writing FFN2's A operand."""
    M, K, lda = _rows(a8)
    N, wk, ldw = _rows(w8)
    qm, qn, ldq = _rows(q_out)
    if wk != K or qm != M or qn != N:
        raise RuntimeError("gemm_fp8_gelu_q: shape mismatch")
    _call("flexam_gemm_fp8_gelu_q", _ptr(a8, U8), lda, _ptr(a_scale, F32), _ptr(w8, U8), ldw, _ptr(w_scale, F32), _ptr(bias, F32),
          _ptr(out_scale, F32), _ptr(q_out, U8), ldq, M, N, K)
    return q_out


def gemm_fp8_gate_residual(a8, a_scale, w8, w_scale, bias, x, gate=None, gate_row=None, rows_per_batch=0):
    """x[M,N] (fp32, in place) += bf16((a8 @ w8^T) * scales + bias) * gate[row]."""
    M, K, lda = _rows(a8)
    N, wk, ldw = _rows(w8)
    xm, xn, ldx = _rows(x)
    if wk != K or xm != M or xn != N:
        raise RuntimeError("gemm_fp8_gate_residual: shape mismatch")
    _call("flexam_gemm_fp8_gate_residual", _ptr(a8, U8), lda, _ptr(a_scale, F32), _ptr(w8, U8), ldw, _ptr(w_scale, F32), _ptr(bias, F32),
          _ptr(x, F32), ldx, _ptr(gate, F32), gate.stride(0) if gate is not None else 0, _ptr(gate_row, I32), rows_per_batch, M, N, K)
    return x


# ----------------------------------------------------------------------------- attention
# The kernels' geometry, from the header (tests/test_abi_cpu.py holds the header to QBLK, KVBLK, HD and REC_BYTES of the sources): a
# work unit is ATTN_Q_BLOCK query rows of one (batch, head), keys go in tiles of ATTN_KV_TILE, an MXFP8 record holds one key tile
ATTN_Q_BLOCK = abi.CONSTANTS["FLEXAM_ATTN_Q_BLOCK"]
ATTN_KV_TILE = abi.CONSTANTS["FLEXAM_ATTN_KV_TILE"]
ATTN_HEAD_DIM = abi.CONSTANTS["FLEXAM_ATTN_HEAD_DIM"]
ATTN8_REC_BYTES = abi.CONSTANTS["FLEXAM_ATTN8_REC_BYTES"]
ATTN_PRESCALED = abi.CONSTANTS["FLEXAM_ATTN_PRESCALED"]


def attn_units(batch_heads: int, lq: int) -> int:
    """Work units of a launch: one per (batch, head) and block of ATTN_Q_BLOCK query rows."""
    return batch_heads * -(-lq // ATTN_Q_BLOCK)


def attn_kv_tiles(lk: int) -> int:
    return -(-lk // ATTN_KV_TILE)


def attn_split_plan(batch_heads: int, lq: int, lk: int, n_cu: int = 256):
    """(kv_splits, split_from_unit) for flexam_attn_fwd_splitkv.  W = batch_heads * ceil(lq/256) work units of ceil(lk/64) key
    tiles; the launch takes ceil(W/n_cu) rounds.  Cutting only the units of the last, partial round into S key ranges turns
    that round into ceil(rem*S/n_cu)/S of a round (+ 4 % per pass for the partial outputs and the merge); S is kept only if the
    whole launch gets more than 2 % shorter and every range keeps at least 8 key tiles."""
    w = attn_units(batch_heads, lq)
    tiles = attn_kv_tiles(lk)
    full, rem = (w // n_cu) * n_cu, w % n_cu
    if rem == 0:
        return 1, w
    best, best_cost = 1, float(w // n_cu + 1)
    for s in (2, 3, 4, 5, 6, 8):
        if tiles // s < 8:
            break
        passes = -(-rem * s // n_cu)
        cost = w // n_cu + passes * (1.0 / s + 0.04)
        if cost < best_cost * 0.98:
            best, best_cost = s, cost
    return (best, full) if best > 1 else (1, w)


def attn_partial_splits(units: int, tiles: int, n_cu: int = 256) -> int:
    """Key ranges per work unit for a partial-attention call: fill whole rounds of the CUs, every range >= 8 key tiles."""
    best, best_cost = 1, float(-(-units // n_cu))
    for s in range(2, 9):
        if tiles // s < 8:
            break
        cost = -(-units * s // n_cu) / s + 0.04
        if cost < best_cost * 0.97:
            best, best_cost = s, cost
    return best


def attn_effective_splits(lk: int, splits: int) -> int:
    """Key ranges a request for `splits` really gives: ranges hold whole 64-key tiles, empty trailing ranges are dropped."""
    tiles = attn_kv_tiles(lk)
    splits = max(1, min(int(splits), tiles))
    per = -(-tiles // splits)
    return -(-tiles // per)


def _packed_heads(who, *tensors):
    """[B, L, H, D] views (None skipped) whose heads lie side by side in a row, as the kernels address them: column h * D."""
    D = tensors[0].shape[3]
    for t in tensors:
        if t is not None and (t.stride(3) != 1 or t.stride(2) != D):
            raise RuntimeError(f"{who}: heads must be packed along the row (stride(2) == head_dim, stride(3) == 1)")


def _softmax_scale(softmax_scale, prescaled, head_dim):
    return ATTN_PRESCALED if prescaled else (softmax_scale if softmax_scale is not None else head_dim ** -0.5)


def _split_request(kv_splits, split_from_unit, batch_heads, lq, lk):
    """(S, from_unit) of a split-KV launch.  kv_splits None: attn_split_plan (only the last, partial round of the CUs is split); an
    explicit kv_splits splits every unit unless split_from_unit is given too."""
    if kv_splits is None:
        return attn_split_plan(batch_heads, lq, lk, num_cus())
    return int(kv_splits), (0 if split_from_unit is None else int(split_from_unit))


def _partials(slots, units, device):
    """(ws_o, ws_ml): per slot, unit and query row the un-normalised output and the (reference, row sum) pair of a partial softmax."""
    return (torch.empty(slots, units, ATTN_Q_BLOCK, ATTN_HEAD_DIM, device=device, dtype=F32),
            torch.empty(slots, units, ATTN_Q_BLOCK, 2, device=device, dtype=F32))


_ATTN_WS = {}


def _split_scratch(device, stream: int, S: int, n: int):
    """(ws_o, ws_ml) of a split-KV launch that cuts n units into S key ranges: per-shape scratch per (device, stream), reused across
    launches (stream-ordered) and re-made when the shape changes."""
    key = _ws_key(device, stream)
    if key in _ATTN_WS and _ATTN_WS[key][0] != (S, n):
        del _ATTN_WS[key]
    return _ws_slot(_ATTN_WS, key, lambda: ((S, n), *_partials(S, n, device)))[1:]


def attn_fwd_lastkey(q, k, v, last_key_multiplicity, out=None, softmax_scale=None, prescaled=False):
    """attn_fwd with the last key counted `last_key_multiplicity` times (identical trailing context rows folded into one, see
    flexam_hip.h); same layouts as attn_fwd, no split-KV (short contexts)."""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    _packed_heads("attn_fwd_lastkey", q, k, v)
    if out is None:
        out = torch.empty(B, Lq, H, D, device=q.device, dtype=BF16)
    _call("flexam_attn_fwd_lastkey", _ptr(q, BF16), q.stride(0), q.stride(1), _ptr(k, BF16), k.stride(0), k.stride(1), _ptr(v, BF16),
          v.stride(0), v.stride(1), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, Lq, Lk, D, _softmax_scale(softmax_scale, prescaled, D),
          float(last_key_multiplicity))
    return out


def attn_fwd(q, k, v, out=None, softmax_scale=None, kv_splits=None, split_from_unit=None, prescaled=False):
    """q [B,Lq,H,128], k/v [B,Lk,H,128] bf16 (arbitrary batch/row strides, head dim contiguous and
    heads packed: stride(2) == 128) -> out [B,Lq,H,128] bf16.  kv_splits None: plan from attn_split_plan (only the last,
    partial round of the CUs is split); an explicit kv_splits splits every unit unless split_from_unit is given too.
    prescaled: q already carries softmax_scale * log2(e) (folded into its producer before the rounding to bf16)."""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    _packed_heads("attn_fwd", q, k, v)
    if out is None:
        out = torch.empty(B, Lq, H, D, device=q.device, dtype=BF16)
    S, from_unit = _split_request(kv_splits, split_from_unit, B * H, Lq, Lk)
    args = (_ptr(q, BF16), q.stride(0), q.stride(1), _ptr(k, BF16), k.stride(0), k.stride(1), _ptr(v, BF16), v.stride(0), v.stride(1),
            _ptr(out, BF16), out.stride(0), out.stride(1), B, H, Lq, Lk, D, _softmax_scale(softmax_scale, prescaled, D))
    if S <= 1:
        _call("flexam_attn_fwd", *args)
        return out
    ws_o, ws_ml = _split_scratch(q.device, _stream(), S, attn_units(B * H, Lq) - from_unit)
    _call("flexam_attn_fwd_splitkv", *args, S, from_unit, _ptr(ws_o, F32), _ptr(ws_ml, F32))
    return out


def attn_window(window, causal=False):
    """(left, right) of flash-attn's mask as two ints, a negative side written -1; causal sets right = 0 as flash-attn does."""
    left, right = (int(w) for w in window)
    return (left if left >= 0 else -1), (0 if causal else right if right >= 0 else -1)


def attn_window_tiles(L: int, window):
    """Per block of ATTN_Q_BLOCK query rows the (first, last) key tile the windowed kernel visits: the tiles that hold a key some row of
    the block sees.  window = (left, right), a negative side unbounded: row i sees key j iff j >= i - left and j <= i + right.  The rows'
    intervals overlap from row to row, so their union is one range of keys: from the first row's first key to the last row's last."""
    left, right = attn_window(window)
    out = []
    for q0 in range(0, L, ATTN_Q_BLOCK):
        q1 = min(q0 + ATTN_Q_BLOCK, L) - 1
        first = 0 if left < 0 else max(0, q0 - left)
        last = L - 1 if right < 0 else min(L - 1, q1 + right)
        out.append((first // ATTN_KV_TILE, last // ATTN_KV_TILE))
    return out


def attn_window_sink_tiles(L: int, window, sink: int):
    """attn_window_tiles with the first `sink` keys visible to every row (row i sees key j iff j < sink or j is in its window): per block
    of ATTN_Q_BLOCK query rows the list of (first, last) key-tile runs the windowed kernel walks -- the sink tiles [0, (sink - 1) // 64]
    and the window tiles of attn_window_tiles, as ONE run where they touch or overlap and as two runs with a gap otherwise."""
    if sink < 0:
        raise ValueError(f"attn_window_sink_tiles: negative sink {sink}")
    n_sink = -(-min(sink, L) // ATTN_KV_TILE)                  # the sink tiles are [0, n_sink)
    out = []
    for first, last in attn_window_tiles(L, window):
        if n_sink == 0:
            out.append([(first, last)])
        elif n_sink >= first:
            out.append([(0, max(last, n_sink - 1))])
        else:
            out.append([(0, n_sink - 1), (first, last)])
    return out


def attn_window_frames_tiles(L: int, window_frames, frame_tokens: int, sink: int = 0):
    """attn_window_sink_tiles for a window counted in frames of `frame_tokens` = T tokens from token 0 (flexam_attn_fwd_window_frames):
    row i sees key j iff j < sink or (a < 0 or j // T >= i // T - a) and (b < 0 or j // T <= i // T + b), window_frames = (a, b).  Per
    block of ATTN_Q_BLOCK query rows the list of (first, last) key-tile runs the windowed kernel walks.  A row's keys are the range
    [(i // T - a) T, (i // T + b + 1) T - 1] clipped to [0, L) and both ends are non-decreasing in i, so a block's window keys run from
    its first row's first key to its last row's last; the sink tiles join them as in attn_window_sink_tiles -- but for a < 0, where the
    entry point drops the sink (nothing lies to the left of such a window) and so does this.  GPU-free."""
    a, b = attn_window(window_frames)
    T, sink = int(frame_tokens), int(sink)
    if T <= 0:
        raise ValueError(f"attn_window_frames_tiles: frame_tokens {frame_tokens} (1 or more)")
    if sink < 0:
        raise ValueError(f"attn_window_frames_tiles: negative sink {sink}")
    n_sink = -(-min(sink, L) // ATTN_KV_TILE) if a >= 0 else 0            # (nothing lies to the left of a window without a left bound)
    out = []
    for q0 in range(0, L, ATTN_Q_BLOCK):
        q1 = min(q0 + ATTN_Q_BLOCK, L) - 1
        first = (0 if a < 0 else max(0, (q0 // T - a) * T)) // ATTN_KV_TILE
        last = (L - 1 if b < 0 else min(L - 1, (q1 // T + b + 1) * T - 1)) // ATTN_KV_TILE
        if n_sink == 0:
            out.append([(first, last)])
        elif n_sink >= first:
            out.append([(0, max(last, n_sink - 1))])
        else:
            out.append([(0, n_sink - 1), (first, last)])
    return out


def attn_window_at_tiles(Lq: int, Lk: int, q_offset: int, window, sink: int = 0, frame_tokens: int = 0):
    """The three planners above for a call at a query offset (flexam_attn_fwd_window_at): row i of Lq is global token g = q_offset + i
    and sees key j of Lk iff j < sink or lo(g) <= j <= hi(g), the bounds in tokens (frame_tokens = 0) or in frames of T = frame_tokens
    tokens, a negative side unbounded (and a negative left side drops the sink, as everywhere).  Per block of ATTN_Q_BLOCK query rows the
    list of (first, last) key-tile runs the kernel walks; [] for a block none of whose rows sees a key (pad rows behind the keys: the
    kernel reads no tile and writes zeros).  Both bounds are non-decreasing in g, so a block's window keys run from its first row's first
    key to its last row's last.  At q_offset = 0, Lq = Lk it is the planner of the form asked for (but for a sink under a token window
    without a left bound, which attn_window_sink_tiles keeps and every entry point drops: this follows the entry points).  GPU-free."""
    a, b = attn_window(window)
    Lq, Lk, q0, sink, T = int(Lq), int(Lk), int(q_offset), int(sink), int(frame_tokens)
    if q0 < 0 or sink < 0 or T < 0:
        raise ValueError(f"attn_window_at_tiles: q_offset {q0}, sink {sink}, frame_tokens {T} (none may be negative)")
    T = max(T, 1)                                              # (a token window is a window of one-token frames)
    n_sink = -(-min(sink, Lk) // ATTN_KV_TILE) if a >= 0 else 0
    out = []
    for r0 in range(0, Lq, ATTN_Q_BLOCK):
        ga, gz = q0 + r0, q0 + min(r0 + ATTN_Q_BLOCK, Lq) - 1
        first = 0 if a < 0 else max(0, (ga // T - a) * T)
        last = Lk - 1 if b < 0 else min(Lk - 1, (gz // T + b + 1) * T - 1)
        runs = [(0, n_sink - 1)] if n_sink else []
        if first <= last:
            first, last = first // ATTN_KV_TILE, last // ATTN_KV_TILE
            if n_sink and n_sink >= first:
                runs = [(0, max(last, n_sink - 1))]
            else:
                runs.append((first, last))
        out.append(runs)
    return out


def attn_fwd_window(q, k, v, window, out=None, softmax_scale=None, prescaled=False, sink=0, frame_tokens=0, q_offset=None,
                    key_gap_tiles=None, Lk=None, k_rows=None):
    """attn_fwd under flash-attn's sliding-window mask (see flexam_hip.h): q, k, v [B, L, H, 128] bf16 with the layouts of attn_fwd and
    ONE length L; window = (left, right), a negative side unbounded, (-1, -1) the ordinary call.  Whole work units only (no split-KV).
    sink > 0: the first `sink` keys stay visible to every row whatever the window says (flexam_attn_fwd_window_sink); sink = 0 is the
    call this function has always made.  frame_tokens = T > 0: `window` = (a, b) counts frames of T tokens from token 0, row i sees the
    frames i // T - a .. i // T + b whole (flexam_attn_fwd_window_frames); frame_tokens = 0 changes no call.
    q_offset (None: the calls above, one length): the Lq rows of q are the global tokens q_offset .. q_offset + Lq - 1 of a sequence whose
    first Lk tokens are the keys (flexam_attn_fwd_window_at: a rank's chunk under sequence parallelism; Lq != Lk is welcome, rows from Lk on
    are pad rows, and a row that sees no key comes back as zeros).
    key_gap_tiles (None: the calls above; with q_offset and Lk): k and v are a COMPACT buffer of k_rows rows (default: all of k's) of a
    sequence of Lk keys -- the sink tiles, then the key tiles from global tile s_n + key_gap_tiles on, as dit_layout.halo_plan lays them
    out (flexam_attn_fwd_window_halo, which refuses a buffer that a query block's tiles do not fit)."""
    B, L, H, D = q.shape
    if key_gap_tiles is not None:
        if q_offset is None or Lk is None:
            raise RuntimeError("attn_fwd_window: a compact key buffer (key_gap_tiles) goes with q_offset and the global key count Lk")
        k_rows = k.shape[1] if k_rows is None else int(k_rows)
        if v.shape[1] != k.shape[1] or k_rows > k.shape[1]:
            raise RuntimeError(f"attn_fwd_window: k_rows = {k_rows} of a compact buffer of {k.shape[1]} key and {v.shape[1]} value rows")
        _packed_heads("attn_fwd_window", q, k, v)
        if out is None:
            out = torch.empty(B, L, H, D, device=q.device, dtype=BF16)
        left, right = attn_window(window)
        _call("flexam_attn_fwd_window_halo", _ptr(q, BF16), q.stride(0), q.stride(1), _ptr(k, BF16), k.stride(0), k.stride(1), _ptr(v, BF16),
              v.stride(0), v.stride(1), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, L, int(Lk), D,
              _softmax_scale(softmax_scale, prescaled, D), left, right, int(frame_tokens), int(sink), int(q_offset), int(key_gap_tiles), k_rows)
        return out
    if q_offset is not None and (int(q_offset) != 0 or k.shape[1] != L):
        Lk = k.shape[1]
        if v.shape[1] != Lk:
            raise RuntimeError(f"attn_fwd_window: keys and values share one length (Lk = {Lk}, Lv = {v.shape[1]})")
        _packed_heads("attn_fwd_window", q, k, v)
        if out is None:
            out = torch.empty(B, L, H, D, device=q.device, dtype=BF16)
        left, right = attn_window(window)
        _call("flexam_attn_fwd_window_at", _ptr(q, BF16), q.stride(0), q.stride(1), _ptr(k, BF16), k.stride(0), k.stride(1), _ptr(v, BF16),
              v.stride(0), v.stride(1), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, L, Lk, D, _softmax_scale(softmax_scale, prescaled, D),
              left, right, int(frame_tokens), int(sink), int(q_offset))
        return out
    if k.shape[1] != L or v.shape[1] != L:
        raise RuntimeError(f"attn_fwd_window: queries and keys share one length (Lq = {L}, Lk = {k.shape[1]})")
    _packed_heads("attn_fwd_window", q, k, v)
    if out is None:
        out = torch.empty(B, L, H, D, device=q.device, dtype=BF16)
    left, right = attn_window(window)
    sink = int(sink)
    args = (_ptr(q, BF16), q.stride(0), q.stride(1), _ptr(k, BF16), k.stride(0), k.stride(1), _ptr(v, BF16), v.stride(0), v.stride(1),
            _ptr(out, BF16), out.stride(0), out.stride(1), B, H, L, D, _softmax_scale(softmax_scale, prescaled, D), left, right)
    if int(frame_tokens) != 0:
        _call("flexam_attn_fwd_window_frames", *args, int(frame_tokens), sink)
    elif sink == 0:
        _call("flexam_attn_fwd_window", *args)
    else:
        _call("flexam_attn_fwd_window_sink", *args, sink)
    return out


def attn_partial_workspace(B, H, Lq, n_slots, device):
    return _partials(n_slots, attn_units(B * H, Lq), device)


def attn_fwd_partial(q, k, v, ws, slot0, kv_splits=1, softmax_scale=None, prescaled=False):
    """Partial softmax of q against THESE keys into workspace slots slot0 .. slot0 + kv_splits - 1 (see flexam_hip.h);
    returns the number of slots written."""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    _packed_heads("attn_fwd_partial", q, k, v)
    S = attn_effective_splits(Lk, kv_splits)
    ws_o, ws_ml = ws
    if slot0 + S > ws_o.shape[0] or ws_o.shape[1] != attn_units(B * H, Lq):
        raise RuntimeError("attn_fwd_partial: workspace too small for these slots / this query shape")
    _call("flexam_attn_fwd_partial", _ptr(q, BF16), q.stride(0), q.stride(1), _ptr(k, BF16), k.stride(0), k.stride(1), _ptr(v, BF16),
          v.stride(0), v.stride(1), B, H, Lq, Lk, D, _softmax_scale(softmax_scale, prescaled, D), S, slot0, _ptr(ws_o, F32), _ptr(ws_ml, F32))
    return S


def attn_merge(out, ws, n_slots, softmax_scale=None, prescaled=False):
    """out [B, Lq, H, 128] bf16 = the softmax over the union of the key sets of workspace slots 0 .. n_slots - 1."""
    B, Lq, H, D = out.shape
    _packed_heads("attn_merge", out)
    _call("flexam_attn_merge", _ptr(out, BF16), out.stride(0), out.stride(1), B, H, Lq, D, _softmax_scale(softmax_scale, prescaled, D),
          n_slots, _ptr(ws[0], F32), _ptr(ws[1], F32))
    return out


def _fp8_operands(B, H, L):
    """(shape, dtype) of q8, qs and kv8 (see flexam_hip.h): e4m3 query rows, four E8M0 scale bytes per row, one record per key tile."""
    lp = attn_units(1, L) * ATTN_Q_BLOCK               # query rows come in whole blocks
    return ((B, H, lp, ATTN_HEAD_DIM), U8), ((B, H, lp), I32), ((B, H, attn_kv_tiles(L), ATTN8_REC_BYTES), U8)


def attn_fp8_buffers(B, H, L, device):
    """(q8, qs, kv8) for attn_fp8_pack / attn_fwd_fp8 at this shape (see flexam_hip.h)."""
    return tuple(torch.zeros(shape, device=device, dtype=dt) for shape, dt in _fp8_operands(B, H, L))      # zeros: rmsnorm_rope_mx never writes the padding rows


def _check_fp8_bufs(bufs, B, H, L, device, who):
    """The MXFP8 operand buffers are raw byte images the C side cannot size-check: refuse anything that is not what attn_fp8_buffers(B,
    H, L) makes (shape, dtype, device, contiguity) -- a buffer set of another (B, L) would be out-of-bounds device traffic, not an
    error.  The kernels also rely on the padding rows past L staying zero, which attn_fp8_buffers' torch.zeros guarantees and nothing
    here ever writes."""
    if not isinstance(bufs, (tuple, list)) or len(bufs) != 3:
        raise RuntimeError(f"{who}: bufs must be the (q8, qs, kv8) triple of attn_fp8_buffers")
    for t, (shape, dt) in zip(bufs, _fp8_operands(B, H, L)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != torch.device(device):
            raise RuntimeError(f"{who}: operand buffers are not attn_fp8_buffers(B={B}, H={H}, L={L}) on {device}: got {tuple(t.shape)} {t.dtype} "
                               f"on {t.device}, want {shape} {dt}")


def _k_shift(who, k_shift, B, C, device, name="k_shift"):
    """The smooth-K shift of the shifted producers (and, under their names, smooth-V's v_shift and o_shift): contiguous fp32 [B, C] on
    the operands' device (see flexam_hip.h)."""
    if (not torch.is_tensor(k_shift) or tuple(k_shift.shape) != (B, C) or k_shift.dtype != F32 or not k_shift.is_contiguous()
            or k_shift.device != torch.device(device)):
        got = f"{tuple(k_shift.shape)} {k_shift.dtype} on {k_shift.device}" if torch.is_tensor(k_shift) else type(k_shift).__name__
        raise RuntimeError(f"{who}: {name} must be contiguous float32 [B={B}, {C}] on {device}, got {got}")
    return _ptr(k_shift, F32)


def k_mean_parts(tokens_per_batch):
    """The parts k_mean cuts a batch's tokens into: a function of the token count alone (never of the device), so that equal inputs give
    equal bits everywhere.  16 tokens per part, at most 512 parts: one wave per part and batch."""
    return max(1, min(-(-tokens_per_batch // 16), 512))


def k_mean(k, wk, rope_cos, rope_sin, tokens_per_batch, token_offset=0, eps=1e-6, head_dim=128, out=None, scratch=None):
    """mean over the tokens of K as the attention will see it -> out fp32 [B, C] (flexam_k_mean): k [M, C] bf16 rows, M = B *
    tokens_per_batch; with wk, RMSNorm over the row + RoPE (rmsnorm_rope's arithmetic, unrounded) are applied first, with wk None k is
    taken as given.  scratch: fp32 [B, parts, C], its second size IS the number of parts (default: k_mean_parts(tokens_per_batch))."""
    M, C, ldk = _rows(k)
    if tokens_per_batch <= 0 or M % tokens_per_batch:
        raise RuntimeError(f"k_mean: {M} rows do not tile batches of {tokens_per_batch} tokens")
    B = M // tokens_per_batch
    if wk is not None:
        if rope_cos is None or rope_sin is None or head_dim != ATTN_HEAD_DIM or C % head_dim:
            raise RuntimeError(f"k_mean: with a norm weight the RoPE tables are mandatory and heads are {ATTN_HEAD_DIM} channels")
        if wk.numel() != C or not wk.is_contiguous():
            raise RuntimeError(f"k_mean: the norm weight must be contiguous float32 [{C}]")
        for t in (rope_cos, rope_sin):
            if t.dim() != 2 or t.shape[1] != head_dim // 2 or not t.is_contiguous() or t.shape[0] < token_offset + tokens_per_batch:
                raise RuntimeError(f"k_mean: RoPE tables must be contiguous float32 [>= {token_offset + tokens_per_batch}, {head_dim // 2}], "
                                   f"got {tuple(t.shape)}")
    if scratch is None:
        scratch = torch.empty(B, k_mean_parts(tokens_per_batch), C, device=k.device, dtype=F32)
    if (scratch.dim() != 3 or scratch.shape[0] != B or scratch.shape[2] != C or not 1 <= scratch.shape[1] <= tokens_per_batch
            or scratch.dtype != F32 or not scratch.is_contiguous() or scratch.device != k.device):
        raise RuntimeError(f"k_mean: scratch must be contiguous float32 [B={B}, 1 <= parts <= {tokens_per_batch}, {C}] on {k.device}, got "
                           f"{tuple(scratch.shape)} {scratch.dtype}")
    if out is None:
        out = torch.empty(B, C, device=k.device, dtype=F32)
    if tuple(out.shape) != (B, C) or out.dtype != F32 or not out.is_contiguous() or out.device != k.device:
        raise RuntimeError(f"k_mean: out must be contiguous float32 [B={B}, {C}] on {k.device}, got {tuple(out.shape)} {out.dtype}")
    norm = wk is not None
    _call("flexam_k_mean", _ptr(k, BF16), ldk, _ptr(wk, F32), M, C, eps, _ptr(rope_cos if norm else None, F32),
          _ptr(rope_sin if norm else None, F32), tokens_per_batch, token_offset, head_dim, scratch.shape[1], _ptr(scratch, F32), _ptr(out, F32))
    return out


def attn_fp8_pack(q, k, v, bufs=None, k_shift=None, v_shift=None):
    """q, k, v [B, L, H, 128] bf16 (q prescaled by softmax_scale * log2 e) -> the MXFP8 operand buffers of attn_fwd_fp8.  k_shift
    (smooth-K, fp32 [B, H * 128]): K is quantised from float(k) - k_shift (flexam_attn_fp8_pack_shift).  v_shift (smooth-V, fp32
    [B, H * 128]): V is quantised from float(v) - v_shift, also in the V-only call (flexam_attn_fp8_pack_shift_kv); attn_fwd_fp8 then
    takes the same tensor as o_shift."""
    B, L, H, D = v.shape
    if any(t is not None and t.shape != v.shape for t in (q, k)):
        raise RuntimeError(f"attn_fp8_pack: q, k, v must be [B, L, H, {ATTN_HEAD_DIM}], all of one shape")
    _packed_heads("attn_fp8_pack", v, q, k)
    if (q is None) != (k is None):
        raise RuntimeError("attn_fp8_pack: q and k go together (both None: V only, after rmsnorm_rope_mx)")
    if bufs is None:
        bufs = attn_fp8_buffers(B, H, L, v.device)
    _check_fp8_bufs(bufs, B, H, L, v.device, "attn_fp8_pack")
    q8, qs, kv8 = bufs
    qk = (lambda t: (t.stride(0), t.stride(1))) if q is not None else (lambda t: (0, 0))
    args = (_ptr(q, BF16), *qk(q), _ptr(k, BF16), *qk(k), _ptr(v, BF16), v.stride(0), v.stride(1), _raw(q8), _raw(qs), _raw(kv8), B, H, L, D)
    if k_shift is not None and k is None:
        raise RuntimeError("attn_fp8_pack: k_shift needs its k")
    ks = _k_shift("attn_fp8_pack", k_shift, B, H * D, v.device) if k_shift is not None else None
    if v_shift is not None:
        _call("flexam_attn_fp8_pack_shift_kv", *args, ks, _k_shift("attn_fp8_pack", v_shift, B, H * D, v.device, "v_shift"))
    elif k_shift is not None:
        _call("flexam_attn_fp8_pack_shift", *args, ks)
    else:
        _call("flexam_attn_fp8_pack", *args)
    return bufs


def rmsnorm_rope_mx(q, wq, k, wk, bufs, rope_cos, rope_sin, tokens_per_batch, token_offset=0, eps=1e-6, heads=24, k_shift=None):
    """RMSNorm + RoPE of q and k ([M, 3072] bf16 views) written as the MXFP8 operands of attn_fwd_fp8 (Q rows, K image and scales);
    the V half of `bufs` comes from attn_fp8_pack(None, None, v, bufs).  k_shift (smooth-K, fp32 [B, 3072]): the K half is that of
    k - k_shift, subtracted behind the rotation (flexam_rmsnorm_rope_mx_shift)."""
    M, C, ldq = _rows(q)
    if tokens_per_batch <= 0 or M % tokens_per_batch or C != heads * ATTN_HEAD_DIM:
        raise RuntimeError(f"rmsnorm_rope_mx: {M} rows of {C} columns do not tile batches of {tokens_per_batch} tokens x {heads} heads x "
                           f"{ATTN_HEAD_DIM}")
    _check_fp8_bufs(bufs, M // tokens_per_batch, heads, tokens_per_batch, q.device, "rmsnorm_rope_mx")
    q8, qs, kv8 = bufs
    args = (_ptr(q, BF16), ldq, _ptr(wq, F32), _ptr(k, BF16), k.stride(0), _ptr(wk, F32), _raw(q8), _raw(qs), _raw(kv8), M, C, eps,
            _ptr(rope_cos, F32), _ptr(rope_sin, F32), tokens_per_batch, token_offset, heads, ATTN_HEAD_DIM)
    if k_shift is None:
        _call("flexam_rmsnorm_rope_mx", *args)
    else:
        _call("flexam_rmsnorm_rope_mx_shift", *args, _k_shift("rmsnorm_rope_mx", k_shift, M // tokens_per_batch, C, q.device))
    return bufs


def _fp8_split_words(device, kv_splits, split_from_unit, batch_heads, lq, lk):
    """(kv_splits, split_from_unit, ws_o, ws_ml) as the MXFP8 entry points take them: 1, 0 and no workspace when nothing is split."""
    S, from_unit = _split_request(kv_splits, split_from_unit, batch_heads, lq, lk)
    if S <= 1:
        return 1, 0, None, None
    ws_o, ws_ml = _split_scratch(device, _stream(), S, attn_units(batch_heads, lq) - from_unit)
    return S, from_unit, _ptr(ws_o, F32), _ptr(ws_ml, F32)


def attn_fwd_fp8(bufs, L, out=None, kv_splits=None, split_from_unit=None, o_shift=None, window=(-1, -1), sink=0, frame_tokens=0):
    """Self-attention from packed MXFP8 operands (attn_fp8_pack) -> out [B, L, H, 128] bf16.  o_shift (smooth-V, fp32 [B, H * 128]: the
    v_shift the operands were packed with) is added to the output in fp32 before its one rounding (flexam_attn_fwd_fp8_oshift).
    window / sink / frame_tokens: attn_fwd_window's mask (flexam_attn_fwd_fp8_window: whole work units, so no kv_splits); the defaults
    make the call this function has always made."""
    q8, qs, kv8 = bufs
    B, H, D = q8.shape[0], q8.shape[1], ATTN_HEAD_DIM
    _check_fp8_bufs(bufs, B, H, L, q8.device, "attn_fwd_fp8")
    if out is None:
        out = torch.empty(B, L, H, D, device=q8.device, dtype=BF16)
    _packed_heads("attn_fwd_fp8", out)
    if tuple(out.shape) != (B, L, H, D):
        raise RuntimeError(f"attn_fwd_fp8: out must be [B={B}, L={L}, H={H}, {D}] with heads packed along the row, got {tuple(out.shape)}")
    shift = _k_shift("attn_fwd_fp8", o_shift, B, H * D, q8.device, "o_shift") if o_shift is not None else None
    left, right = attn_window(window)
    if (left, right) != (-1, -1):
        if kv_splits is not None:
            raise RuntimeError("attn_fwd_fp8: a window runs whole work units (no kv_splits)")
        _call("flexam_attn_fwd_fp8_window", _raw(q8), _raw(qs), _raw(kv8), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, L, D,
              left, right, int(sink), int(frame_tokens), shift)
        return out
    args = (_raw(q8), _raw(qs), _raw(kv8), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, L, D,
            *_fp8_split_words(q8.device, kv_splits, split_from_unit, B * H, L, L))
    if o_shift is None:
        _call("flexam_attn_fwd_fp8", *args)
    else:
        _call("flexam_attn_fwd_fp8_oshift", *args, shift)
    return out


def attn_fwd_fp8_chunked(q8, qs, kv8_chunks, lq, lk, out=None, window=(-1, -1), sink=0, frame_tokens=0, q_offset=0, o_shift=None):
    """Attention of `lq` local queries (q8 / qs of attn_fp8_buffers(B, H, lq)) over `lk` keys whose MXFP8 records come in CHUNKS:
    kv8_chunks uint8 [n_chunks, B, H, chunk_tiles, ATTN8_REC_BYTES], chunk c holding the keys [c, c + 1) * chunk_tiles * 64 -- the
    rank-major result of all-gathering every sequence-parallel rank's own records.  -> out [B, lq, H, 128] bf16.
    window / sink / frame_tokens / q_offset: attn_fwd_window's mask with row i of the call as global token q_offset + i
    (flexam_attn_fwd_fp8_window_at: whole work units; a row that sees no key is zeros); o_shift goes with a window only.  The defaults
    make the call this function has always made."""
    B, H, D = q8.shape[0], q8.shape[1], ATTN_HEAD_DIM
    for t, (shape, dt) in zip((q8, qs), _fp8_operands(B, H, lq)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"attn_fwd_fp8_chunked: q8 / qs are not the query buffers of attn_fp8_buffers(B={B}, H={H}, L={lq})")
    if (kv8_chunks.dim() != 5 or kv8_chunks.dtype != U8 or not kv8_chunks.is_contiguous() or tuple(kv8_chunks.shape[1:3]) != (B, H)
            or kv8_chunks.shape[4] != ATTN8_REC_BYTES or kv8_chunks.device != q8.device):
        raise RuntimeError(f"attn_fwd_fp8_chunked: records must be contiguous uint8 [chunks, B={B}, H={H}, chunk_tiles, {ATTN8_REC_BYTES}], got {tuple(kv8_chunks.shape)}")
    n_chunks, chunk_tiles = kv8_chunks.shape[0], kv8_chunks.shape[3]
    if not 0 < lk <= n_chunks * chunk_tiles * ATTN_KV_TILE:
        raise RuntimeError(f"attn_fwd_fp8_chunked: {lk} keys do not fit {n_chunks} chunks of {chunk_tiles} tiles")
    if out is None:
        out = torch.empty(B, lq, H, D, device=q8.device, dtype=BF16)
    _packed_heads("attn_fwd_fp8_chunked", out)
    if tuple(out.shape) != (B, lq, H, D):
        raise RuntimeError(f"attn_fwd_fp8_chunked: out must be [B={B}, L={lq}, H={H}, {D}] with heads packed along the row, got {tuple(out.shape)}")
    left, right = attn_window(window)
    if (left, right) != (-1, -1):
        shift = _k_shift("attn_fwd_fp8_chunked", o_shift, B, H * D, q8.device, "o_shift") if o_shift is not None else None
        _call("flexam_attn_fwd_fp8_window_at", _raw(q8), _raw(qs), _raw(kv8_chunks), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, lq, lk,
              chunk_tiles, D, left, right, int(sink), int(frame_tokens), int(q_offset), shift)
        return out
    if o_shift is not None:
        raise RuntimeError("attn_fwd_fp8_chunked: o_shift goes with a window (the unmasked chunked call takes none)")
    _call("flexam_attn_fwd_fp8_chunked", _raw(q8), _raw(qs), _raw(kv8_chunks), _ptr(out, BF16), out.stride(0), out.stride(1), B, H, lq, lk,
          chunk_tiles, D, *_fp8_split_words(q8.device, None, None, B * H, lq, lk))
    return out


# ----------------------------------------------------------------------------- DiT row kernels
def ln_modulate(x, out=None, eps=1e-6, shift=None, scale=None, row_index=None, rows_per_batch=0, ln_w=None, ln_b=None):
    M, C, ldx = _rows(x)
    if out is None:
        out = torch.empty(M, C, device=x.device, dtype=BF16)
    tab_ld = shift.stride(0) if shift is not None else 0
    if shift is not None and (shift.stride(-1) != 1 or scale.stride(-1) != 1 or scale.stride(0) != tab_ld):
        raise RuntimeError("ln_modulate: shift/scale must be row views of one table")
    _call("flexam_ln_modulate", _ptr(x, F32), ldx, M, C, eps, _ptr(shift, F32), _ptr(scale, F32), tab_ld, _ptr(row_index, I32),
          rows_per_batch, _ptr(ln_w, F32), _ptr(ln_b, F32), _ptr(out, BF16), out.stride(0))
    return out


def ln_modulate_fp8(x, q_out, row_scale, eps=1e-6, shift=None, scale=None, row_index=None, rows_per_batch=0, ln_w=None, ln_b=None,
                    next_scale=None, next_wnorm=0.0, next_bias=0.0):
    """ln_modulate with the output written as e4m3 bytes q_out [M, C] (uint8, row stride free) + row_scale [M] fp32.  next_scale [M]
    (optional): the output scale of the GEMM + GELU this row feeds (gemm_fp8_gelu_q), from the row's L2 norm and the bounds
    next_wnorm >= max |w_j|_2, next_bias >= max |b_j| of that GEMM (see flexam_hip.h)."""
    M, C, ldx = _rows(x)
    tab_ld = shift.stride(0) if shift is not None else 0
    _call("flexam_ln_modulate_fp8", _ptr(x, F32), ldx, M, C, eps, _ptr(shift, F32), _ptr(scale, F32), tab_ld, _ptr(row_index, I32),
          rows_per_batch, _ptr(ln_w, F32), _ptr(ln_b, F32), _ptr(q_out, torch.uint8), q_out.stride(0), _ptr(row_scale, F32),
          _ptr(next_scale, F32), float(next_wnorm), float(next_bias))
    return q_out, row_scale


def gate_residual(x, y, gate=None, row_index=None, rows_per_batch=0):
    M, C, ldx = _rows(x)
    gate_ld = gate.stride(0) if gate is not None else 0
    _call("flexam_gate_residual", _ptr(x, F32), ldx, _ptr(y, BF16), y.stride(0), _ptr(gate, F32), gate_ld, _ptr(row_index, I32),
          rows_per_batch, M, C)
    return x


def rmsnorm_rope(q, wq, k=None, wk=None, eps=1e-6, rope_cos=None, rope_sin=None, tokens_per_batch=0, token_offset=0,
                 head_dim=128, q_out=None, k_out=None):
    """In place by default.  q/k: 2-D bf16 views [M, C]."""
    M, C, ldq = _rows(q)
    q_out = q if q_out is None else q_out
    k_out = k if k_out is None else k_out
    _call("flexam_rmsnorm_rope", _ptr(q, BF16), ldq, _ptr(q_out, BF16), q_out.stride(0), _ptr(wq, F32), _ptr(k, BF16),
          k.stride(0) if k is not None else 0, _ptr(k_out, BF16), k_out.stride(0) if k_out is not None else 0, _ptr(wk, F32), M, C, eps,
          _ptr(rope_cos, F32), _ptr(rope_sin, F32), tokens_per_batch, token_offset, head_dim)
    return q_out, k_out


def rmsnorm_rope_scatter(q, wq, k, wk, v, q_out, k_out, v_out, ld_out, out_bs, col_block, block_stride, eps=1e-6, rope_cos=None,
                         rope_sin=None, tokens_per_batch=0, token_offset=0, head_dim=128):
    """q/k/v: 2-D bf16 views [M, C] (q, v optional); *_out: bf16 tensors whose data pointers are the bases of the scattered
    layout described in flexam_hip.h (element (m, col) -> (m // tpb) * out_bs + (m % tpb) * ld_out + (col // col_block) *
    block_stride + col % col_block)."""
    M, C, ldk = _rows(k)
    _call("flexam_rmsnorm_rope_scatter", _ptr(q, BF16), q.stride(0) if q is not None else 0, _ptr(wq, F32), _ptr(k, BF16), ldk,
          _ptr(wk, F32), _ptr(v, BF16), v.stride(0) if v is not None else 0, _ptr(q_out, BF16), _ptr(k_out, BF16), _ptr(v_out, BF16),
          ld_out, out_bs, col_block, block_stride, M, C, eps, _ptr(rope_cos, F32), _ptr(rope_sin, F32), tokens_per_batch, token_offset,
          head_dim)


# (scale_mask, dens_slots) of the model's two AdaLN tables: a block's six slots (shift, scale, gate of the attention and the FFN half:
# bit j of scale_mask set = slot j is a scale and gets + 1; nibble j of dens_slots = the density slot added to slot j, 0xF = none) and the
# head's two (shift, scale)
ModSlots = namedtuple("ModSlots", "scale_mask dens_slots")
MOD_BLOCK_SLOTS = ModSlots(0b010010, 0xFF1FF0)
MOD_HEAD_SLOTS = ModSlots(0b10, 0xF0)


def mod_table(mod, e, out, rows_per_batch, scale_mask, mdens=None, dens=None, dens_slots=-1):
    """mod [nblk,nj,C], e [R,nj,C], mdens [nblk,nslot,C], dens [B,nslot,C] -> out [nblk,R,nj,C] fp32."""
    nblk, nj, C = mod.shape
    R = e.shape[0]
    nslot = mdens.shape[1] if mdens is not None else 0
    for t in (mod, e, out, mdens, dens):
        if t is not None and not t.is_contiguous():
            raise RuntimeError("mod_table: tensors must be contiguous")
    _call("flexam_mod_table", _ptr(mod, F32), _ptr(e, F32), _ptr(mdens, F32), _ptr(dens, F32), _ptr(out, F32), nblk, R, nj, nslot, C,
          rows_per_batch, scale_mask, dens_slots)
    return out


def small_linear(x, w, b=None, silu_in=False, out=None):
    """fp32 y[M,N] = silu?(x[M,K]) @ w[N,K]^T + b, M <= 32; w bf16 or fp32 (each output sums in the same order whatever M is)."""
    M, K, ldx = _rows(x)
    N, wk, ldw = _rows(w)
    if wk != K:
        raise RuntimeError("small_linear: K mismatch")
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=F32)
    if w.dtype not in (BF16, F32):
        raise RuntimeError("small_linear: weight must be bf16 or fp32")
    _call("flexam_small_linear_f32", _ptr(x, F32), ldx, _ptr(w), 1 if w.dtype == BF16 else 0, ldw, _ptr(b, F32), _ptr(out, F32),
          out.stride(0), M, N, K, 1 if silu_in else 0)
    return out


def sinusoid_embed(t, dim, out=None):
    R = t.numel()
    if out is None:
        out = torch.empty(R, dim, device=t.device, dtype=F32)
    _call("flexam_sinusoid_embed", _ptr(t.contiguous(), F32), _ptr(out, F32), R, dim)
    return out


def patchify(src, dst, col0=0, row0=0):
    """src [C,F,H,W] (fp32/bf16, contiguous) -> dst[row0 + token, col0 + c*4+ph*2+pw] (bf16 2-D)."""
    C, F, H, W = src.shape
    if not src.is_contiguous():
        raise RuntimeError("patchify: src must be contiguous")
    _call("flexam_patchify", _ptr(src), 1 if src.dtype == BF16 else 0, C, F, H, W, _ptr(dst, BF16), dst.stride(0), col0, row0)
    return dst


def unpatchify(tok, tok0, C, F, H, W, out=None, dtype=F32):
    if out is None:
        out = torch.empty(C, F, H, W, device=tok.device, dtype=dtype)
    _call("flexam_unpatchify", _ptr(tok, F32), tok.stride(0), tok0, C, F, H, W, _ptr(out), 1 if out.dtype == BF16 else 0)
    return out


def cfg_euler_blend(tok_uncond, tok_cond, tok0, guidance, dt, latents, known=None, mask=None):
    C, F, H, W = latents.shape
    _call("flexam_cfg_euler_blend", _ptr(tok_uncond, F32), _ptr(tok_cond, F32), tok_uncond.stride(0), tok0, guidance, dt,
          _ptr(latents, F32), _ptr(known, F32), _ptr(mask, F32), C, F, H, W)
    return latents


def axpby(y, a, x, b):
    """y = a*x + b*y (fp32, same shape, contiguous)."""
    if y.shape != x.shape or not y.is_contiguous() or not x.is_contiguous():
        raise RuntimeError("axpby: contiguous tensors of equal shape required")
    _call("flexam_axpby_f32", _ptr(y, F32), a, _ptr(x, F32), b, y.numel())
    return y


def checksum(t: torch.Tensor):
    """Content fingerprint (two 64-bit sums of per-(index, word) hashes) of a device tensor; synchronises (host logic only)."""
    return checksums([t])[0]


def checksums(tensors):
    """Fingerprints of several device tensors with ONE readback: every launch adds into its own slot of one buffer."""
    ts = [t.contiguous() for t in tensors]
    if not ts:
        return []
    out = torch.zeros(len(ts), 2, device=ts[0].device, dtype=I64)
    for i, t in enumerate(ts):
        _call("flexam_checksum", _ptr(t), t.numel() * t.element_size(), out[i].data_ptr())
    return [tuple(r) for r in out.tolist()]


def cfg_velocity(tok_uncond, tok_cond, tok0, guidance, out):
    """out [C,F,H,W] fp32 = unpatchify(u + g (c - u)); tok_cond None: out = unpatchify(u)."""
    C, F, H, W = out.shape
    _call("flexam_cfg_velocity", _ptr(tok_uncond, F32), _ptr(tok_cond, F32), tok_uncond.stride(0), tok0, guidance, _ptr(out, F32), C, F, H,
          W)
    return out


def lincomb(out, terms):
    """out = sum(c * t for c, t in terms): fp32 contiguous tensors of out's shape; out may be one of them."""
    n = len(terms)
    for _, t in terms:
        if t.shape != out.shape or t.dtype != F32 or not t.is_contiguous() or t.device != out.device:
            raise RuntimeError("lincomb: fp32 contiguous tensors of equal shape on one device required")
    if not out.is_contiguous() or out.dtype != F32:
        raise RuntimeError("lincomb: out must be fp32 contiguous")
    ptrs = (c_void_p * n)(*[t.data_ptr() for _, t in terms])
    coefs = (c_float * n)(*[float(c) for c, _ in terms])
    _call("flexam_lincomb_f32", _ptr(out, F32), out.numel(), n, ctypes.cast(ptrs, c_void_p), ctypes.cast(coefs, c_void_p))
    return out


def mask_blend(x, known, mask):
    """x [C, ...] = (1 - mask) * known + mask * x with mask [...] broadcast over the leading channel dim."""
    C = x.shape[0]
    fhw = x.numel() // C
    if mask.numel() != fhw or known.shape != x.shape:
        raise RuntimeError("mask_blend: shape mismatch")
    _call("flexam_mask_blend_f32", _ptr(x, F32), _ptr(known, F32), _ptr(mask, F32), C, fhw)
    return x


# ----------------------------------------------------------------------------- channels-last conv helpers
def pack_cl(src, dst, c0=0):
    """src [C,F,H,W] -> interior of dst [F,H+2,W+2,Cp] (bf16) at channel offset c0."""
    C, F, H, W = src.shape
    if not src.is_contiguous() or dst.shape[:3] != (F, H + 2, W + 2) or not dst.is_contiguous():
        raise RuntimeError("pack_cl: bad layout")
    _call("flexam_pack_cl", _ptr(src), 1 if src.dtype == BF16 else 0, C, F, H, W, _ptr(dst, BF16), dst.shape[3], c0)
    return dst


def unpack_cl(src, C, F, H, W, out=None):
    """src [F*(H+2)*(W+2), ld] (fp32/bf16 rows) -> [C,F,H,W] fp32."""
    if out is None:
        out = torch.empty(C, F, H, W, device=src.device, dtype=F32)
    _call("flexam_unpack_cl", _ptr(src), 1 if src.dtype == BF16 else 0, src.stride(0), C, F, H, W, _ptr(out, F32))
    return out


def groupnorm_silu_cl(x, C, F, H, W, groups, gamma, beta, dst, residual=None, eps=1e-5, stats=None):
    """x [F*(H+2)*(W+2), ld] fp32 -> dst [F,H+2,W+2,Cp] bf16 interior; residual: bf16 padded image."""
    if stats is None:
        stats = torch.empty(2 * groups, device=x.device, dtype=F32)
    _call("flexam_groupnorm_silu_cl", _ptr(x, F32), x.stride(0), C, F, H, W, groups, eps, _ptr(gamma, F32), _ptr(beta, F32),
          _ptr(stats, F32), _ptr(residual, BF16), residual.shape[-1] if residual is not None else 0, _ptr(dst, BF16), dst.shape[-1])
    return dst


# ----------------------------------------------------------------------------- VAE decoder helpers
def vae_prep_cl(src, C, T, H, W, dst, mode=0, gamma=None, t0=0, compact=False):
    """src rows [T*(H+2)*(W+2), ld] (fp32/bf16) -> dst image [*, H+2, W+2, Cp] (frame offset t0) or compact [T*H*W, Cp]."""
    _call("flexam_vae_prep_cl", _ptr(src), 1 if src.dtype == BF16 else 0, src.stride(0), C, T, H, W, _ptr(gamma, F32), mode,
          _ptr(dst, BF16), dst.shape[-1], t0, 1 if compact else 0)
    return dst


def upsample2x_cl(src, C, T, H, W, dst, interleave=False):
    _call("flexam_upsample2x_cl", _ptr(src), 1 if src.dtype == BF16 else 0, src.stride(0), C, T, H, W, 1 if interleave else 0,
          _ptr(dst, BF16), dst.shape[-1])
    return dst


def dupup_add_cl(x_main, Co, To, Ho, Wo, x_in, Ci, ft, drop):
    _call("flexam_dupup_add_cl", _ptr(x_main, F32), x_main.stride(0), Co, To, Ho, Wo, _ptr(x_in, F32), x_in.stride(0), Ci, ft, drop)
    return x_main


def deinterleave_cl(src, C, T, H, W, dst):
    """src rows [T*(H+2)*(W+2), 2C] -> dst padded image [2T, H+2, W+2, Cp]: frame 2t + s = channels [sC, (s+1)C) of frame t."""
    _call("flexam_deinterleave_cl", _ptr(src), 1 if src.dtype == BF16 else 0, src.stride(0), C, T, H, W, _ptr(dst, BF16), dst.shape[-1])
    return dst


def phase_dupup_cl(phases, x_main, Co, To, Ho, Wo, x_in, Ci, ft, drop):
    """phases [4, rows of the padded (Ho/2, Wo/2) image, Co] fp32 -> x_main rows of the padded (Ho, Wo) image, + the DupUp3D shortcut of x_in."""
    if phases.dim() != 3 or phases.shape[0] != 4 or phases.stride(2) != 1 or phases.shape[2] != Co:
        raise RuntimeError("phase_dupup_cl: phases must be [4, rows, Co] fp32")
    _call("flexam_phase_dupup_cl", _ptr(phases, F32), phases.stride(1), phases.stride(0), _ptr(x_main, F32), x_main.stride(0), Co, To, Ho,
          Wo, _ptr(x_in, F32), x_in.stride(0), Ci, ft, drop)
    return x_main


def tapsum_cl(y, T, H, W, kt, Co, bias, out):
    """y [(kt - 1 + T) * (H+2) * (W+2), >= kt*9*Co] fp32 per-tap products -> out rows [T * (H+2) * (W+2), Co] fp32 (interior positions)."""
    _call("flexam_tapsum_cl", _ptr(y, F32), y.stride(0), T, H, W, kt, Co, _ptr(bias, F32), _ptr(out, F32), out.stride(0))
    return out


def softmax_rows(s, scale, out, n_valid):
    M = s.shape[0]
    _call("flexam_softmax_rows", _ptr(s, F32), s.stride(0), M, n_valid, scale, _ptr(out, BF16), out.stride(0), out.shape[1])
    return out


def scatter_add_cl(x, y, C, T, H, W):
    _call("flexam_scatter_add_cl", _ptr(x, F32), x.stride(0), _ptr(y, BF16), y.stride(0), C, T, H, W)
    return x


def vae_unpatchify_clamp(src, T, H, W, video, f0, lo=-1.0, hi=1.0):
    _call("flexam_vae_unpatchify_clamp", _ptr(src, F32), src.stride(0), T, H, W, _ptr(video, F32), video.shape[1], f0, lo, hi)
    return video


def pack_affine_cl(src, mul, add, dst):
    C, T, H, W = src.shape
    _call("flexam_pack_affine_cl", _ptr(src.contiguous(), F32), C, T, H, W, _ptr(mul, F32), _ptr(add, F32), _ptr(dst, BF16), dst.shape[-1])
    return dst


# ----------------------------------------------------------------------------- VAE encoder helpers
def vae_patchify_cl(video, f0, T, dst, t0=0):
    """video [3, Ftot, 2H, 2W] fp32 frames f0..f0+T -> dst image [*, H+2, W+2, Cp] frames t0.., 12 channels (c r q)."""
    _, ftot, h2, w2 = video.shape
    _call("flexam_vae_patchify_cl", _ptr(video, F32), ftot, f0, T, h2 // 2, w2 // 2, _ptr(dst, BF16), dst.shape[-1], t0)
    return dst


def space_to_depth_cl(src, C, T, H, W, dst, Cs, t0=0):
    """src rows [T*(H+2)*(W+2), ld] -> dst image [*, H/2+2, W/2+2, 4*Cs]."""
    _call("flexam_space_to_depth_cl", _ptr(src), 1 if src.dtype == BF16 else 0, src.stride(0), C, T, H, W, _ptr(dst, BF16), Cs, t0)
    return dst


def avgdown_add_cl(x_main, Co, To, Ho, Wo, x_in, Ci, Ti, ft, fs):
    _call("flexam_avgdown_add_cl", _ptr(x_main, F32), x_main.stride(0), Co, To, Ho, Wo, _ptr(x_in, F32), x_in.stride(0), Ci, Ti, ft, fs)
    return x_main


# ----------------------------------------------------------------------------- umT5 text encoder helpers
def t5_norm(x, w, out, eps=1e-6):
    """x [M, C] fp32 rows -> out [M, C] (bf16 or fp32) = w * x * rsqrt(mean(x^2) + eps)."""
    M, C, ldx = _rows(x)
    _call("flexam_t5_norm", _ptr(x, F32), ldx, M, C, eps, _ptr(w, F32), _ptr(out), out.stride(0), 1 if out.dtype == F32 else 0)
    return out


def softmax_bias_rows(s, out, n_valid, scale=1.0, bias=None, key_mask=None):
    """out [M, Npad] bf16 = softmax(scale * s[:, :n_valid] + bias) over keys with key_mask != 0 (uniform over the n_valid keys when
    every key is masked, as in the reference); columns n_valid .. Npad are 0."""
    M = s.shape[0]
    _call("flexam_softmax_bias_rows", _ptr(s, F32), s.stride(0), M, n_valid, scale, _ptr(bias, F32),
          bias.stride(0) if bias is not None else 0, _ptr(key_mask, F32), _ptr(out, BF16), out.stride(0), out.shape[1])
    return out


def mul_bf16(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    if a.shape != b.shape or not (a.is_contiguous() and b.is_contiguous() and out.is_contiguous()):
        raise RuntimeError("mul_bf16: contiguous bf16 tensors of equal shape required")
    _call("flexam_mul_bf16", _ptr(a, BF16), _ptr(b, BF16), _ptr(out, BF16), a.numel())
    return out


# ----------------------------------------------------------------------------- conditioning rasteriser (csrc/raster.hip)
def raster_keys(points, visible, height, width, half, y_min=0, mask=None, keys=None):
    """points [T, N, 3] fp32 (u, v, depth), visible [T, N] uint8 / bool or None, mask [T, H, W] fp32 or None -> keys [T, H, W] int64
    (the uint64 key image of flexam_raster_keys: per pixel the nearest drawn point, all ones = none)."""
    if points.dim() != 3 or points.shape[2] != 3 or not points.is_contiguous():
        raise RuntimeError(f"raster_keys: contiguous points [T, N, 3] required, got {tuple(points.shape)}")
    T, N, _ = points.shape
    if visible is not None:
        if visible.dtype == torch.bool:
            visible = visible.view(U8)
        if visible.shape != (T, N) or not visible.is_contiguous():
            raise RuntimeError(f"raster_keys: visible must be contiguous [T, N] = {(T, N)}, got {tuple(visible.shape)}")
    if mask is not None and (mask.shape != (T, height, width) or not mask.is_contiguous()):
        raise RuntimeError(f"raster_keys: mask must be contiguous [T, H, W] = {(T, height, width)}, got {tuple(mask.shape)}")
    if keys is None:
        keys = torch.empty(T, height, width, device=points.device, dtype=torch.int64)
    elif keys.shape != (T, height, width) or keys.dtype != torch.int64 or not keys.is_contiguous():
        raise RuntimeError("raster_keys: keys must be a contiguous int64 [T, H, W] buffer")
    _call("flexam_raster_keys", _ptr(points, F32), _ptr(visible, U8), T, N, height, width, half, y_min, _ptr(mask, F32), _ptr(keys))
    keys.raster_points = N                         # the point count these keys index: raster_resolve holds its colour table to it
    return keys


def raster_resolve(keys, colors, out_u8=None, out_f32=None, want_u8=False, want_f32=True, n_points=None):
    """keys [T, H, W] (raster_keys), colors [N, 3] or [T, N, 3] uint8 -> (bytes [T, H, W, 3] or None, planes [3, T, H, W] fp32 = byte / 255 or None).
    N must be the point count the keys were made with (raster_keys attaches it to its result; `n_points` for keys from elsewhere): a
    shorter table would be read past its end, a longer per-frame one at another frame's rows."""
    T, H, W = keys.shape
    n_keys = n_points if n_points is not None else getattr(keys, "raster_points", None)
    if colors.dtype != U8 or colors.shape[-1] != 3 or not colors.is_contiguous() or colors.dim() not in (2, 3):
        raise RuntimeError(f"raster_resolve: contiguous uint8 colours [N, 3] or [T, N, 3] required, got {tuple(colors.shape)} {colors.dtype}")
    if colors.dim() == 3 and colors.shape[0] != T:
        raise RuntimeError("raster_resolve: per-frame colours need one table per frame")
    stride = colors.shape[1] * 3 if colors.dim() == 3 else 0
    N = colors.shape[-2]
    if n_keys is not None and N != n_keys:
        raise RuntimeError(f"raster_resolve: the keys index {n_keys} points, the colour table has {N} rows")
    if out_u8 is None and want_u8:
        out_u8 = torch.empty(T, H, W, 3, device=keys.device, dtype=U8)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(3, T, H, W, device=keys.device, dtype=F32)
    for o, shp in ((out_u8, (T, H, W, 3)), (out_f32, (3, T, H, W))):
        if o is not None and (tuple(o.shape) != shp or not o.is_contiguous()):
            raise RuntimeError(f"raster_resolve: output must be contiguous {shp}, got {tuple(o.shape)}")
    _call("flexam_raster_resolve", _ptr(keys, torch.int64), _ptr(colors, U8), stride, N, T, H, W, _ptr(out_u8, U8), _ptr(out_f32, F32))
    return out_u8, out_f32


# ----------------------------------------------------------------------------- foreground-edit masks (csrc/edit_mask.hip)
EDIT_MASK_SLOTS = 48          # frames the hull stage works on at once: its scratch is 5 * H * ceil(W / 2) ints per frame


def _frames_u8(t, what):
    if t.dim() != 3 or t.dtype != U8 or not t.is_contiguous():
        raise RuntimeError(f"{what}: contiguous uint8 frames [n, H, W] required, got {tuple(t.shape)} {t.dtype}")
    return t.shape


def edit_mask_blur(src, weights, out=None):
    """src [n, H, W] uint8 in {0, 1}, weights [r + 1] float64 (gaussian_filter's normalised kernel from its centre outwards) ->
    out [n, H, W] uint8 = blurred > 0.5, with scipy.ndimage.gaussian_filter's arithmetic."""
    n, H, W = _frames_u8(src, "edit_mask_blur")
    if weights.dim() != 1 or weights.dtype != torch.float64 or not weights.is_contiguous() or weights.device != src.device:
        raise RuntimeError("edit_mask_blur: weights must be a contiguous float64 vector on the frames' device")
    if out is None:
        out = torch.empty_like(src)
    elif tuple(out.shape) != (n, H, W) or out.dtype != U8 or not out.is_contiguous():
        raise RuntimeError(f"edit_mask_blur: out must be contiguous uint8 {(n, H, W)}")
    tmp = torch.empty(n, H, W, device=src.device, dtype=F32)
    _call("flexam_edit_mask_blur", _ptr(src, U8), n, H, W, _ptr(weights, torch.float64), weights.numel() - 1, _ptr(tmp, F32), _ptr(out, U8))
    return out


def edit_mask_hull(binary):
    """binary [n, H, W] uint8 -> (runs [n, H, ceil(W / 2)] int32, nruns [n, H] int32): per run slot the (lo | hi << 16) interval its
    8-connected component's filled convex hull covers in its row (lo > hi: none)."""
    n, H, W = _frames_u8(binary, "edit_mask_hull")
    S = (W + 1) // 2
    runs = torch.empty(n, H, S, device=binary.device, dtype=torch.int32)
    nruns = torch.empty(n, H, device=binary.device, dtype=torch.int32)
    slots = min(n, EDIT_MASK_SLOTS)
    ws = torch.empty(slots, 5, H, S, device=binary.device, dtype=torch.int32)
    _call("flexam_edit_mask_hull", _ptr(binary, U8), n, H, W, _ptr(runs, torch.int32), _ptr(nruns, torch.int32), _raw(ws), slots)
    return runs, nruns


def edit_mask_dilate(runs, nruns, width, half_widths, out=None):
    """runs / nruns of edit_mask_hull, half_widths [r + 1] int32 (the element's row half widths, |dy| = 0 .. r) -> out [n, H, W] uint8
    in {0, 1}: the intervals dilated by the element."""
    if runs.dim() != 3 or runs.dtype != torch.int32 or not runs.is_contiguous() or runs.shape[2] != (width + 1) // 2:
        raise RuntimeError(f"edit_mask_dilate: runs must be contiguous int32 [n, H, ceil(W / 2)] for W = {width}, got {tuple(runs.shape)}")
    n, H, _ = runs.shape
    if tuple(nruns.shape) != (n, H) or nruns.dtype != torch.int32 or not nruns.is_contiguous():
        raise RuntimeError(f"edit_mask_dilate: nruns must be contiguous int32 {(n, H)}")
    if half_widths.dim() != 1 or half_widths.dtype != torch.int32 or not half_widths.is_contiguous() or half_widths.device != runs.device:
        raise RuntimeError("edit_mask_dilate: half_widths must be a contiguous int32 vector on the runs' device")
    if out is None:
        out = torch.empty(n, H, width, device=runs.device, dtype=U8)
    elif tuple(out.shape) != (n, H, width) or out.dtype != U8 or not out.is_contiguous():
        raise RuntimeError(f"edit_mask_dilate: out must be contiguous uint8 {(n, H, width)}")
    _call("flexam_edit_mask_dilate", _ptr(runs, torch.int32), _ptr(nruns, torch.int32), n, H, width, _ptr(half_widths, torch.int32),
          half_widths.numel() - 1, _ptr(out, U8))
    return out


# ----------------------------------------------------------------------------- frames across the boundary (csrc/frames.hip)
FRAMES_MAX_TAPS = abi.CONSTANTS["FLEXAM_FRAMES_MAX_TAPS"]


def _tap_table(table, n_out, n_in, device, what):
    index, weights = table
    if tuple(index.shape) != (n_out, 2) or index.dtype != I32 or not index.is_contiguous() or index.device != device:
        raise RuntimeError(f"{what}: tap index must be contiguous int32 [{n_out}, 2] on {device}, got {tuple(index.shape)} {index.dtype}")
    if weights.dim() != 2 or weights.shape[0] != n_out or weights.dtype != F32 or not weights.is_contiguous() or weights.device != device:
        raise RuntimeError(f"{what}: tap weights must be contiguous float32 [{n_out}, k] on {device}, got {tuple(weights.shape)} {weights.dtype}")
    k = weights.shape[1]
    if not 1 <= k <= min(FRAMES_MAX_TAPS, n_in):
        raise RuntimeError(f"{what}: {k} taps per output, 1 .. min({FRAMES_MAX_TAPS}, source size {n_in}) allowed")
    return index, weights, k


def frames_resize(src, dst, y_table, x_table, mul=1.0, div=1.0, add=0.0):
    """src: (t, c, y, x) view [T, C, H, W], uint8 or float32, any non-negative strides; dst: (t, c, y, x) view [T, C, oh, ow] float32 with
    contiguous columns; *_table = (index [n_out, 2] int32 (first, count), weights [n_out, k] float32) as flexam_amd.frames builds them.
    dst = resize(src) * mul / div + add (flexam_frames_resize)."""
    if src.dim() != 4 or src.dtype not in (U8, F32) or not src.is_cuda:
        raise RuntimeError(f"frames_resize: a uint8 or float32 GPU view [T, C, H, W] is required, got {tuple(src.shape)} {src.dtype} on {src.device}")
    T, C, H, W = src.shape
    if dst.dim() != 4 or dst.dtype != F32 or dst.device != src.device or dst.shape[:2] != (T, C) or (dst.shape[3] > 1 and dst.stride(3) != 1):
        raise RuntimeError(f"frames_resize: dst must be a float32 view [{T}, {C}, oh, ow] with contiguous columns on {src.device}, got "
                           f"{tuple(dst.shape)} {dst.dtype} stride {dst.stride()}")
    oh, ow = dst.shape[2:]
    if min(T, C, H, W, oh, ow) < 1 or min(src.stride() + dst.stride()) < 0:
        raise RuntimeError(f"frames_resize: empty frames or negative strides: {tuple(src.shape)} -> {tuple(dst.shape)}")
    if float(div) == 0.0:
        raise RuntimeError("frames_resize: div = 0")
    yi, yw, ky = _tap_table(y_table, oh, H, src.device, "frames_resize (y)")
    xi, xw, kx = _tap_table(x_table, ow, W, src.device, "frames_resize (x)")
    _call("flexam_frames_resize", _ptr(src), int(src.dtype == U8), *src.stride(), T, C, H, W, _ptr(dst, F32), *dst.stride()[:3], oh, ow,
          _ptr(yi, I32), _ptr(yw, F32), ky, _ptr(xi, I32), _ptr(xw, F32), kx, float(mul), float(div), float(add))
    return dst


def frames_to_bytes(video, signed=True, out=None):
    """video [C, T, H, W] float32 or bf16, contiguous, C <= 4 -> out [T, H, W, C] uint8 (flexam_frames_to_bytes): signed: x / 2 + 0.5
    first; clamp to [0, 1], * 255, truncation; NaN -> 0."""
    if video.dim() != 4 or video.dtype not in (F32, BF16) or not video.is_contiguous() or not 1 <= video.shape[0] <= 4 or video.numel() == 0:
        raise RuntimeError(f"frames_to_bytes: a contiguous float32 or bf16 clip [C <= 4, T, H, W] is required, got {tuple(video.shape)} {video.dtype}")
    C, T, H, W = video.shape
    if out is None:
        out = torch.empty(T, H, W, C, device=video.device, dtype=U8)
    elif tuple(out.shape) != (T, H, W, C) or out.dtype != U8 or not out.is_contiguous() or out.device != video.device:
        raise RuntimeError(f"frames_to_bytes: out must be contiguous uint8 {(T, H, W, C)} on {video.device}")
    _call("flexam_frames_to_bytes", _ptr(video), int(video.dtype == BF16), C, T, H, W, int(bool(signed)), _ptr(out, U8))
    return out


# ----------------------------------------------------------------------------- edit tracks: camera / object motion (csrc/motion.hip)
MOTION_CHUNK = abi.CONSTANTS["FLEXAM_MOTION_CHUNK"]
F64 = torch.float64


def _points3(t, what, dims=(2, 3), dtypes=(F32,)):
    if t.dim() not in dims or t.shape[-1] != 3 or t.dtype not in dtypes or not t.is_contiguous():
        raise RuntimeError(f"{what}: contiguous points [..., 3] of {dtypes} required, got {tuple(t.shape)} {t.dtype}")
    return t


def _bytes_mask(m, shape, what):
    if m.dtype == torch.bool:
        m = m.view(U8)
    if m.dtype != U8 or tuple(m.shape) != tuple(shape) or not m.is_contiguous():
        raise RuntimeError(f"{what}: contiguous bool / uint8 mask {tuple(shape)} required, got {tuple(m.shape)} {m.dtype}")
    return m


def _motion_select(name, points, mask, extra):
    n = points.shape[0]
    flags = torch.empty(n, device=points.device, dtype=U8)
    ws = torch.empty(4 * ((n + MOTION_CHUNK - 1) // MOTION_CHUNK), device=points.device, dtype=F64)
    sums = torch.empty(4, device=points.device, dtype=F64)
    _call(name, _ptr(points, F32), n, _ptr(mask, U8), *extra, _ptr(flags, U8), _raw(ws), ws.numel() * 8, _ptr(sums, F64))
    return flags.view(torch.bool), sums


def motion_select_map(points, mask):
    """points [N, 3] fp32, mask [N] bool -> (flags [N] bool = mask & no NaN coordinate, sums [4] fp64 = sum x, y, z and the number of the
    flagged points, in a fixed summation order)."""
    _points3(points, "motion_select_map", dims=(2,))
    return _motion_select("flexam_motion_select_map", points, _bytes_mask(mask, (points.shape[0],), "motion_select_map"), ())


def motion_select_pixels(points, mask):
    """points [N, 3] fp32 (first-frame pixel positions), mask [Hm, Wm] bool -> (flags [N] = the mask at the rounded, clamped positions, sums)."""
    _points3(points, "motion_select_pixels", dims=(2,))
    if mask.dim() != 2:
        raise RuntimeError(f"motion_select_pixels: mask [Hm, Wm] required, got {tuple(mask.shape)}")
    return _motion_select("flexam_motion_select_pixels", points, _bytes_mask(mask, mask.shape, "motion_select_pixels"), tuple(mask.shape))


def motion_compact(mask):
    """mask [N] bool -> (index [N] int32 whose first `count` entries are the set positions in ascending order, count [1] int32), both on the device."""
    if mask.dim() != 1:
        raise RuntimeError(f"motion_compact: mask [N] required, got {tuple(mask.shape)}")
    mask = _bytes_mask(mask, mask.shape, "motion_compact")
    n = mask.numel()
    index = torch.empty(n, device=mask.device, dtype=I32)
    count = torch.empty(1, device=mask.device, dtype=I32)
    ws = torch.empty((n + MOTION_CHUNK - 1) // MOTION_CHUNK, device=mask.device, dtype=I32)
    _call("flexam_motion_compact", _ptr(mask, U8), n, _ptr(index, I32), _ptr(count, I32), _raw(ws), ws.numel() * 4)
    return index, count


def _rows34(m, T, rows, cols, dtype, what):
    if m is None:
        return None
    if tuple(m.shape) != (T, rows, cols) or m.dtype != dtype or not m.is_contiguous():
        raise RuntimeError(f"{what}: contiguous {dtype} [{T}, {rows}, {cols}] required, got {tuple(m.shape)} {m.dtype}")
    return m


def motion_transform(src, T, flags=None, motion=None, pose=None, intr=None, scale=(1.0, 1.0), index=None, count=None, out=None):
    """src [T, N, 3] or [N, 3] (one map for all T frames) fp32 -> out [T, M, 3]: object affine motion [T, 3, 4] on the flagged points (all
    when flags is None), camera pose [T, 3, 4] + intrinsics [3, 3] + perspective division, (u, v) scale, gathered through index[:count]
    (M = count; without an index M = N).  See flexam_motion_transform_f32."""
    _points3(src, "motion_transform")
    n = src.shape[-2]
    stride = 0 if src.dim() == 2 else n * 3
    if src.dim() == 3 and src.shape[0] != T:
        raise RuntimeError(f"motion_transform: {src.shape[0]} source frames for T = {T}")
    if flags is not None:
        flags = _bytes_mask(flags, (n,), "motion_transform")
    motion = _rows34(motion, T, 3, 4, F32, "motion_transform: motion")
    pose = _rows34(pose, T, 3, 4, F32, "motion_transform: pose")
    if intr is not None and (tuple(intr.shape) != (3, 3) or intr.dtype != F32 or not intr.is_contiguous()):
        raise RuntimeError(f"motion_transform: intr must be contiguous fp32 [3, 3], got {tuple(intr.shape)} {intr.dtype}")
    if index is not None and (index.dtype != I32 or index.dim() != 1 or index.numel() < count or not index.is_contiguous()):
        raise RuntimeError("motion_transform: index must be a contiguous int32 vector of at least `count` entries")
    m = n if index is None else int(count)
    if out is None:
        out = torch.empty(T, m, 3, device=src.device, dtype=F32)
    elif tuple(out.shape) != (T, m, 3) or out.dtype != F32 or not out.is_contiguous():
        raise RuntimeError(f"motion_transform: out must be contiguous fp32 {(T, m, 3)}")
    if m == 0:
        return out
    _call("flexam_motion_transform_f32", _ptr(src, F32), stride, T, n, _ptr(flags, U8), _ptr(motion, F32), _ptr(pose, F32), _ptr(intr, F32),
          float(scale[0]), float(scale[1]), _ptr(index, I32), m, _ptr(out, F32))
    return out


def motion_unproject(points, kinv, rinv, tvec):
    """s2w_vggt's point arithmetic: points [T, N, 3] fp32 or fp64 (u, v, z), kinv / rinv [T, 3, 3], tvec [T, 3] fp64 -> world points in the
    dtype of `points` (computed in double); z <= 0 gives zeros."""
    _points3(points, "motion_unproject", dims=(3,), dtypes=(F32, F64))
    T, n, _ = points.shape
    _rows34(kinv, T, 3, 3, F64, "motion_unproject: kinv")
    _rows34(rinv, T, 3, 3, F64, "motion_unproject: rinv")
    if tuple(tvec.shape) != (T, 3) or tvec.dtype != F64 or not tvec.is_contiguous():
        raise RuntimeError(f"motion_unproject: tvec must be contiguous fp64 {(T, 3)}")
    out = torch.empty_like(points)
    _call("flexam_motion_unproject_f64", _ptr(points), int(points.dtype == F32), T, n, _ptr(kinv, F64), _ptr(rinv, F64), _ptr(tvec, F64), _ptr(out))
    return out


def motion_project(points, pose, intr):
    """w2s_vggt's point arithmetic: world points [T, N, 3] fp32 or fp64, pose [T, 3, 4], intr [T, 3, 3] fp64 -> (u, v, depth) fp64; depth <= 0 gives zeros."""
    _points3(points, "motion_project", dims=(3,), dtypes=(F32, F64))
    T, n, _ = points.shape
    _rows34(pose, T, 3, 4, F64, "motion_project: pose")
    _rows34(intr, T, 3, 3, F64, "motion_project: intr")
    out = torch.empty(T, n, 3, device=points.device, dtype=F64)
    _call("flexam_motion_project_f64", _ptr(points), int(points.dtype == F32), T, n, _ptr(pose, F64), _ptr(intr, F64), _ptr(out, F64))
    return out


# ----------------------------------------------------------------------------- colour tables of the conditioning videos (csrc/raster_colors.hip)
SELECT_MAX_RANKS = abi.CONSTANTS["FLEXAM_SELECT_MAX_RANKS"]
SELECT_WS_SEGMENT_BYTES = abi.CONSTANTS["FLEXAM_SELECT_WS_SEGMENT_BYTES"]


def select_ranks(src, comp, segments, seg_len, ranks=None, mask=None, inverse=False):
    """Exact order statistics of float32 values on the device (flexam_select_f32).  src: contiguous fp32 [..., C]; value (s, i) is
    component `comp` of row s * seg_len + i, through 1 / (x + 1e-10) when `inverse`; mask: bool / uint8 with one entry per row of the
    segments, None = all valid; ranks: int64 [segments, K] on the device, or None to count only.
    -> (values fp32 [segments, K] or None, info int64 [segments, 4] = valid count, a valid NaN, a valid value != 0 before the transform, 0)."""
    if src.dim() < 1 or src.dtype != F32 or not src.is_contiguous():
        raise RuntimeError(f"select_ranks: contiguous fp32 values [..., C] required, got {tuple(src.shape)} {src.dtype}")
    stride = src.shape[-1]
    rows = segments * seg_len
    if segments <= 0 or seg_len <= 0 or stride == 0 or rows > src.numel() // stride:
        raise RuntimeError(f"select_ranks: {segments} segments of {seg_len} rows from {src.numel() // max(stride, 1)} rows")
    if mask is not None:
        mask = mask.view(U8) if mask.dtype == torch.bool else mask
        if mask.dtype != U8 or not mask.is_contiguous() or mask.numel() < rows:
            raise RuntimeError(f"select_ranks: a contiguous bool / uint8 mask of at least {rows} entries required, got {tuple(mask.shape)} {mask.dtype}")
    values, k = None, 0
    if ranks is not None:
        if ranks.dim() != 2 or ranks.shape[0] != segments or ranks.dtype != I64 or not ranks.is_contiguous() or ranks.device != src.device:
            raise RuntimeError(f"select_ranks: ranks must be contiguous int64 [{segments}, K] on the values' device, got {tuple(ranks.shape)} {ranks.dtype}")
        k = ranks.shape[1]
        values = torch.empty(segments, k, device=src.device, dtype=F32)
    info = torch.empty(segments, 4, device=src.device, dtype=I64)
    ws = torch.empty(segments * SELECT_WS_SEGMENT_BYTES // 4, device=src.device, dtype=I32)
    _call("flexam_select_f32", _ptr(src, F32), stride, int(comp), int(bool(inverse)), _ptr(mask, U8), segments, seg_len, _ptr(ranks, I64), k,
          _ptr(values, F32), _ptr(info, I64), _raw(ws), ws.numel() * 4)
    return values, info


def select_lerp(values, gamma, info, f32_form):
    """values fp32 [S, 2 Q] = (lower, upper) pairs of select_ranks, gamma fp64 [S, Q], info of the same select_ranks call -> the
    percentiles [S, Q] with numpy's `_lerp` arithmetic: fp32 (`f32_form`, np.percentile with a scalar q) or fp64 (an array q)."""
    S = values.shape[0]
    if values.dim() != 2 or values.shape[1] % 2 or values.dtype != F32 or not values.is_contiguous():
        raise RuntimeError(f"select_lerp: contiguous fp32 values [S, 2 Q] required, got {tuple(values.shape)} {values.dtype}")
    Q = values.shape[1] // 2
    if tuple(gamma.shape) != (S, Q) or gamma.dtype != F64 or not gamma.is_contiguous() or tuple(info.shape) != (S, 4) or not info.is_contiguous():
        raise RuntimeError(f"select_lerp: gamma must be contiguous fp64 {(S, Q)} and info int64 {(S, 4)}")
    out = torch.empty(S, Q, device=values.device, dtype=F32 if f32_form else F64)
    _call("flexam_select_lerp", _ptr(values, F32), _ptr(gamma, F64), _ptr(info, I64), S, Q, int(bool(f32_form)), _ptr(out))
    return out


def raster_colors_tracking(first_frame, height, width, pct=None, blue=None):
    """first_frame [N, 3] fp32 (u, v, depth), pct fp32 [2] = the (2nd, 98th) percentile of its inverse depths, or blue uint8 [N] -> colours uint8 [N, 3]."""
    _points3(first_frame, "raster_colors_tracking", dims=(2,))
    n = first_frame.shape[0]
    if (pct is None) == (blue is None):
        raise RuntimeError("raster_colors_tracking: either the percentiles or the blue channel")
    if pct is not None and (pct.numel() != 2 or pct.dtype != F32 or not pct.is_contiguous()):
        raise RuntimeError("raster_colors_tracking: pct must be 2 contiguous fp32 values")
    if blue is not None and (tuple(blue.shape) != (n,) or blue.dtype != U8 or not blue.is_contiguous()):
        raise RuntimeError(f"raster_colors_tracking: blue must be contiguous uint8 {(n,)}")
    out = torch.empty(n, 3, device=first_frame.device, dtype=U8)
    _call("flexam_raster_colors_tracking", _ptr(first_frame, F32), n, height, width, _ptr(pct, F32), _ptr(blue, U8), _ptr(out, U8))
    return out


def raster_colors_depth(points, visible, pct, lut):
    """points [T, N, 3] fp32, visible [T, N] bool / uint8 or None, pct fp64 [T, 2] (per-frame 2nd / 98th percentile of the visible
    depths), lut uint8 [258, 3] -> colours uint8 [T, N, 3]; rows of invisible points are 0."""
    _points3(points, "raster_colors_depth", dims=(3,))
    T, n, _ = points.shape
    if visible is not None:
        visible = _bytes_mask(visible, (T, n), "raster_colors_depth")
    if tuple(pct.shape) != (T, 2) or pct.dtype != F64 or not pct.is_contiguous():
        raise RuntimeError(f"raster_colors_depth: pct must be contiguous fp64 {(T, 2)}")
    if tuple(lut.shape) != (258, 3) or lut.dtype != U8 or not lut.is_contiguous():
        raise RuntimeError("raster_colors_depth: lut must be contiguous uint8 [258, 3]")
    out = torch.empty(T, n, 3, device=points.device, dtype=U8)
    _call("flexam_raster_colors_depth", _ptr(points, F32), _ptr(visible, U8), T, n, _ptr(pct, F64), _ptr(lut, U8), _ptr(out, U8))
    return out


def raster_colors_cosine(code):
    """code [N, 3] fp32 (one frame of a cosine encoding) -> colours uint8 [N, 3] = clip((code + 1) / 2, 0, 1) * 255, truncated."""
    _points3(code, "raster_colors_cosine", dims=(2,))
    out = torch.empty(code.shape[0], 3, device=code.device, dtype=U8)
    _call("flexam_raster_colors_cosine", _ptr(code, F32), code.shape[0], _ptr(out, U8))
    return out


# ----------------------------------------------------------------------------- LoRA merge (csrc/lora.hip)
_LORA_CODES = {BF16: abi.CONSTANTS["FLEXAM_LORA_BF16"], F32: abi.CONSTANTS["FLEXAM_LORA_F32"], F8: abi.CONSTANTS["FLEXAM_LORA_E4M3"]}


def lora_merge(w, up, down, scale):
    """w [N, K] (bf16, float32 or float8_e4m3fn; rows contiguous, any row stride >= K: a row range of a fused buffer is fine) +=
    scale * up [N, r] @ down [r, K] in place (flexam_lora_merge): factors both float32 or both bf16, fp32 products and sums over j
    ascending, one rounding to w's dtype (e4m3 saturates at +-448).  Unmerge: the same call with -scale."""
    for name, t in (("w", w), ("up", up), ("down", down)):
        if not torch.is_tensor(t) or t.dim() != 2 or not t.is_cuda:
            raise RuntimeError(f"lora_merge: {name} must be a 2-D GPU tensor, got "
                               f"{(tuple(t.shape), t.dtype, str(t.device)) if torch.is_tensor(t) else type(t)}")
        if t.numel() == 0 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise RuntimeError(f"lora_merge: {name} must be non-empty with contiguous rows that do not overlap, got shape "
                               f"{tuple(t.shape)} stride {t.stride()}")
    if w.dtype not in _LORA_CODES:
        raise RuntimeError(f"lora_merge: w is stored as bf16, float32 or float8_e4m3fn, not {w.dtype}")
    if up.dtype not in (F32, BF16) or down.dtype != up.dtype:
        raise RuntimeError(f"lora_merge: up and down must both be float32 or both bf16, got {up.dtype} and {down.dtype}")
    if up.device != w.device or down.device != w.device:
        raise RuntimeError(f"lora_merge: w on {w.device}, up on {up.device}, down on {down.device}")
    (N, K), r = w.shape, up.shape[1]
    if up.shape[0] != N or tuple(down.shape) != (r, K):
        raise RuntimeError(f"lora_merge: w {tuple(w.shape)} needs up [{N}, r] and down [r, {K}], got {tuple(up.shape)} and {tuple(down.shape)}")
    ld = lambda t: max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]
    _call("flexam_lora_merge", _ptr(w), _LORA_CODES[w.dtype], ld(w), N, K, _ptr(up), _LORA_CODES[up.dtype], ld(up), _ptr(down),
          _LORA_CODES[down.dtype], ld(down), r, float(scale))
    return w
