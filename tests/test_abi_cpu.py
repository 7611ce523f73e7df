"""CPU: the C-ABI library builds for gfx950, loads without a GPU, and exports exactly the entry
points include/flexam_hip.h declares (no compute calls here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "flexam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flexam_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def libpath():
    from flexam_amd import build
    if not os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(build.LIB):
        return build.LIB
    return build.build(verbose=False)


def test_header_declares_the_hot_path_entry_points():
    syms = declared_symbols()
    for must in ("flexam_gemm_bf16", "flexam_attn_fwd", "flexam_rmsnorm_rope", "flexam_ln_modulate", "flexam_gate_residual",
                 "flexam_patchify", "flexam_unpatchify", "flexam_cfg_euler_blend", "flexam_version", "flexam_arch",
                 "flexam_last_error"):
        assert must in syms


def test_library_exports_every_declared_symbol(libpath):
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath], text=True)
    exported = set(re.findall(r" T (flexam_[a-z0-9_]+)", out))
    missing = [s for s in declared_symbols() if s not in exported]
    assert not missing, f"declared in include/flexam_hip.h but not exported: {missing}"
    undeclared = sorted(exported - set(declared_symbols()))
    assert not undeclared, f"exported but not declared in the header: {undeclared}"


def test_ctypes_binding_covers_header_and_loads(libpath):
    from flexam_amd import hip
    assert sorted(hip._SIGNATURES) == declared_symbols()
    lib = hip.load_library(libpath)
    assert lib.flexam_version() >= 1
    assert lib.flexam_arch() == b"gfx950"


def test_code_object_targets_gfx950(libpath):
    data = open(libpath, "rb").read()
    assert b"gfx950" in data and b"gfx942" not in data and b"sm_" not in data


def test_no_cpu_fallback_without_gpu():
    """Product ops must fail loudly on CPU tensors rather than route through torch or the oracle."""
    import torch
    from flexam_amd import hip
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        hip.gemm(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(4, 64, dtype=torch.bfloat16))


def test_replay_table_follows_the_header_and_the_binding(libpath):
    """Command lists (csrc/replay.hip): the committed dispatch table is what flexam_amd/gen_replay.py makes of the header; every
    stream-ordered entry point has an id, the ids are the header order, and the argument kinds the generator derives from the C
    prototypes are the ones the ctypes binding declares (pointer / integer / float per position) -- a recorded call is replayed with
    exactly the words it was made with."""
    import ctypes
    from flexam_amd import gen_replay, hip
    header = open(os.path.join(ROOT, "include", "flexam_hip.h")).read()
    assert open(gen_replay.OUT).read() == gen_replay.generate(header), "csrc/replay_table.inc is stale: python -m flexam_amd.gen_replay"
    lib = hip.load_library(libpath)
    kinds = gen_replay.arg_kinds(header)
    assert lib.flexam_fn_count() == len(kinds) >= 50
    of = {hip._P: "p", hip._I: "i", hip._L: "i", hip._F: "f"}
    for i, name in enumerate(kinds):
        assert lib.flexam_fn_id(name.encode()) == i and lib.flexam_fn_name(i) == name.encode()
        argtypes = hip._SIGNATURES[name][0]
        assert argtypes[-1] is hip._P and "".join(of[t] for t in argtypes[:-1]) == kinds[name], name
        assert len(argtypes) - 1 <= hip.REPLAY_MAX_ARGS
    for name, (argtypes, _) in hip._SIGNATURES.items():             # and nothing that takes a stream is missing from the table
        if argtypes and argtypes[-1] is hip._P and name not in kinds:
            assert name in ("flexam_replay",), name
    assert lib.flexam_fn_id(b"flexam_last_error") == -1 and lib.flexam_fn_id(b"flexam_replay") == -1
    assert ctypes.sizeof(hip._Cmd) == 8 + 8 * hip.REPLAY_MAX_ARGS
    # argument checks of the list itself run without a GPU: an empty list is fine, a wrong id / word count is refused before any launch
    failed = ctypes.c_int64(7)
    assert lib.flexam_replay(None, 0, ctypes.byref(failed), None) == 0 and failed.value == -1
    cmds = (hip._Cmd * 2)()
    cmds[0].fn, cmds[0].nargs = lib.flexam_fn_count(), 0
    assert lib.flexam_replay(cmds, 1, ctypes.byref(failed), None) == -1 and failed.value == 0 and b"unknown" not in lib.flexam_last_error()
    cmds[0].fn, cmds[0].nargs = lib.flexam_fn_id(b"flexam_axpby_f32"), 2                  # takes 5 words + the stream
    assert lib.flexam_replay(cmds, 1, ctypes.byref(failed), None) == -1 and b"flexam_axpby_f32" in lib.flexam_last_error()
    # a well-formed command reaches the entry point's own argument check (null pointers: refused there, index reported)
    cmds[1].fn, cmds[1].nargs = lib.flexam_fn_id(b"flexam_gemm_bf16"), 15
    cmds[0].fn, cmds[0].nargs = cmds[1].fn, 15
    rc = lib.flexam_replay(cmds, 2, ctypes.byref(failed), None)
    assert rc == -1 and failed.value == 0 and b"gemm: null pointer" in lib.flexam_last_error()


def test_recorder_builds_the_words_the_call_was_made_with(libpath, monkeypatch):
    """hip.record() without a GPU: a stand-in library function is 'called' through the recorder and the plan holds one C segment whose
    words equal the arguments (pointer, integers, a float), minus the stream; host_op splits segments; failures are not recorded."""
    import ctypes
    from flexam_amd import hip
    lib = hip.load_library(libpath)
    calls = []

    class Fake:
        def __getattr__(self, name):
            real = getattr(lib, name)
            if name != "flexam_axpby_f32":
                return real
            def f(*a):
                calls.append(a)
                return 0 if a[0] else -1
            return f
    monkeypatch.setattr(hip, "_lib", Fake())
    marks = []
    with hip.record() as plan:
        assert hip.recording()
        hip.lib().flexam_axpby_f32(4096, 1.5, 8192, -2.0, 77, 1234)
        hip.host_op(lambda: marks.append("host"))
        hip.lib().flexam_axpby_f32(0, 1.0, 0, 1.0, 1, 1234)                      # fails (rc -1): executed, not recorded
        hip.lib().flexam_axpby_f32(16, 0.25, 32, 0.0, 5, 1234)
        assert hip.lib().flexam_last_error is lib.flexam_last_error              # queries pass through
    assert not hip.recording() and len(calls) == 3 and marks == ["host"]
    assert [k for k, _, _ in plan.items] == ["c", "py", "c"] and plan.launches == 2
    seg = plan.items[0][1]
    assert seg[0].fn == lib.flexam_fn_id(b"flexam_axpby_f32") and seg[0].nargs == 5
    assert (seg[0].a[0].p, seg[0].a[1].f, seg[0].a[2].p, seg[0].a[3].f, seg[0].a[4].i) == (4096, 1.5, 8192, -2.0, 77)
    seg2 = plan.items[2][1]
    assert (seg2[0].a[0].p, seg2[0].a[1].f, seg2[0].a[4].i) == (16, 0.25, 5)


def test_binding_is_derived_from_the_header_type_for_type():
    """hip._SIGNATURES comes from flexam_amd/abi.py's parse of the header.  Literal expectations for entry points that together cover
    the whole type vocabulary and the awkward spots (24 mixed arguments, adjacent floats, `const char*` in and out, no parameters)."""
    from ctypes import c_char_p, c_float as F, c_int as I, c_int64 as L, c_void_p as P
    from flexam_amd import hip
    want = {
        "flexam_rmsnorm_rope_scatter": ([P, L, P, P, L, P, P, L, P, P, P, L, L, I, L, L, I, F, P, P, L, L, I, P], I),
        "flexam_attn_fwd_lastkey": ([P, L, L, P, L, L, P, L, L, P, L, L, I, I, I, I, I, F, F, P], I),
        "flexam_axpby_f32": ([P, F, P, F, L, P], I),
        "flexam_fn_id": ([c_char_p], I),
        "flexam_fn_name": ([I], c_char_p),
        "flexam_last_error": ([], c_char_p),
        "flexam_version": ([], I),
        "flexam_replay": ([P, L, P, P], I),
    }
    for name, sig in want.items():
        assert hip._SIGNATURES[name] == sig, name
    assert (hip._P, hip._I, hip._L, hip._F) == (P, I, L, F)


def test_int_and_int64_positions_follow_the_header():
    """A c_int where the header says int64_t truncates a stride without failing: for every entry point, the positions the header types
    `int64_t` are c_int64 in the binding and the `int` ones c_int -- read from the header text here, not through the parser."""
    from ctypes import c_int, c_int64
    from flexam_amd import hip
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "flexam_hip.h")).read(), flags=re.S)
    found = re.findall(r"\b(flexam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert [n for n, _ in found] == list(hip._SIGNATURES), "binding keys are the header's prototypes, in header order"
    n64 = n32 = 0
    for name, params in found:
        params = [" ".join(p.split()) for p in params.split(",")] if params.strip() not in ("", "void") else []
        argtypes = hip._SIGNATURES[name][0]
        assert len(argtypes) == len(params), name
        for j, prm in enumerate(params):
            if re.fullmatch(r"int64_t \w+", prm):
                assert argtypes[j] is c_int64, (name, j, prm)
                n64 += 1
            elif re.fullmatch(r"int \w+", prm):
                assert argtypes[j] is c_int, (name, j, prm)
                n32 += 1
            else:
                assert argtypes[j] not in (c_int, c_int64), (name, j, prm)
    assert n64 >= 150 and n32 >= 200, (n64, n32)


@pytest.mark.parametrize("proto", ["int flexam_bad(double x, void* stream);", "int flexam_bad(const void* p, unsigned n);",
                                   "int flexam_bad(size_t n);", "int flexam_bad(flexam_arg a, void* stream);",
                                   "int flexam_bad(const int n);", "int flexam_bad(int32_t n);", "int flexam_bad(int);",
                                   "double flexam_bad(int n);", "void* flexam_bad(void);", "int64_t flexam_bad(void);",
                                   "int flexam_bad(int (*cb)(int), void* stream);"])
def test_parser_refuses_types_outside_the_vocabulary(proto):
    """The vocabulary is closed (int, int64_t, float, const char*, pointers; int or const char* returned): anything else raises with
    the function's name instead of falling back to some ctypes default."""
    from flexam_amd import abi
    ok = "int flexam_ok(const float* const* t, int64_t n, float f, const char* s, void* stream);\n"
    assert [n for n, _, _ in abi.prototypes(ok)] == ["flexam_ok"]
    with pytest.raises(ValueError, match="flexam_bad"):
        abi.prototypes(ok + proto)


def test_header_constants_are_read_not_evaluated():
    from flexam_amd import abi, hip
    c = abi.constants("#define A 3\n#define B (-2)\n#define C (-1.0f)\n#define D (256 * 262144)  /* note */\n#define GUARD\n")
    assert c == {"A": 3, "B": -2, "C": -1.0, "D": 67108864} and isinstance(c["C"], float) and isinstance(c["D"], int)
    for bad in ("#define X (1 << 20)", "#define X sizeof(int)", "#define X 1.0", "#define X (2 + 2)", "#define X Y"):
        with pytest.raises(ValueError, match="X"):
            abi.constants(bad + "\n")
    assert (hip.EPI_NONE, hip.EPI_GELU_TANH, hip.GEMM_WS_BYTES, hip.REPLAY_MAX_ARGS, hip.ATTN_PRESCALED) == (0, 1, 64 << 20, 26, -1.0)
    assert abi.CONSTANTS["FLEXAM_E_ARG"] == -1 and abi.CONSTANTS["FLEXAM_HIP_VERSION"] == 2


def test_attention_geometry_constants_are_the_kernels():
    """The header's attention geometry -- what hip.py and the engine size split-KV workspaces and MXFP8 buffers from -- against the
    constexprs the kernels are compiled with, read from the sources by name: a renamed or re-valued constant fails here, it does not
    mis-size a buffer."""
    from flexam_amd import abi, hip
    ties = (("FLEXAM_ATTN_Q_BLOCK", "attn.hip", "QBLK"), ("FLEXAM_ATTN_KV_TILE", "attn.hip", "KVBLK"),
            ("FLEXAM_ATTN_HEAD_DIM", "attn.hip", "HD"), ("FLEXAM_ATTN8_REC_BYTES", "attn_fp8.inc", "REC_BYTES"))
    for macro, source, name in ties:
        text = open(os.path.join(ROOT, "flexam_amd", "csrc", source)).read()
        found = re.findall(rf"^constexpr int\b[^;]*?\b{name} = (\d+)\s*[,;]", text, flags=re.M)
        assert len(found) == 1, f"csrc/{source}: `constexpr int {name} = <integer>` found {len(found)} times"
        assert int(found[0]) == abi.CONSTANTS[macro], f"{macro} = {abi.CONSTANTS[macro]}, csrc/{source} has {name} = {found[0]}"
    assert (hip.ATTN_Q_BLOCK, hip.ATTN_KV_TILE, hip.ATTN_HEAD_DIM, hip.ATTN8_REC_BYTES) == tuple(abi.CONSTANTS[m] for m, _, _ in ties)


def test_recorder_takes_recordable_from_the_header(libpath):
    """What a recorder records is what the generator makes replayable -- the header's stream-ordered prototypes -- except
    flexam_lincomb_f32, which reads host arrays during the call."""
    from flexam_amd import abi, gen_replay, hip
    header = open(abi.HEADER).read()
    assert hip._REPLAYABLE == set(gen_replay.arg_kinds(header)) and hip._STREAM_ORDERED == hip._REPLAYABLE | {"flexam_replay"}
    assert hip._NOT_RECORDABLE == ("flexam_lincomb_f32",) and "flexam_lincomb_f32" in hip._REPLAYABLE
    lib = hip.load_library(libpath)
    with hip.record():
        with pytest.raises(RuntimeError, match="host arrays"):
            hip.lib().flexam_lincomb_f32
        assert hip.lib().flexam_device_cus is lib.flexam_device_cus and hip.lib().flexam_replay is lib.flexam_replay
        assert hip.lib().flexam_mul_bf16 is not lib.flexam_mul_bf16
