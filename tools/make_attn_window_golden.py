"""Writes tests/golden/attn_window_reference.safetensors: what the REFERENCE's own attention() (FlexAM/models/attention_utils.py:174-233)
returns on the CPU, through its torch-SDPA branch, for the masks flexam_amd serves in HIP -- is_causal=True for the causal case, and a
boolean attn_mask built by flash-attn's window rule (tests/attn_window_cases.allowed) for two windows.  The inputs are those of the
70-token case of tests/attn_window_cases.py in fp32 (B = 1, H = 2); only the outputs are stored, the test rebuilds the inputs.
tests/test_attn_window_cases_cpu.py holds the float64 restatement of tests/attn_window_cases.py to them at fp32 rounding.

`attention` is cut out of the reference's attention_utils.py BY NAME with `ast` at run time and executed with the flash-attn and
SageAttention switches off (the technique of tools/make_golden_lora.py: the module's own imports need packages this build does not have);
the reference's code runs, nothing of it is stored here.  Needs the reference checkout (FLEXAM_REFERENCE_ROOT, as oracle/ref_raster.py
reads it); never imported by flexam_amd, bench.py or the tests.

    python tools/make_attn_window_golden.py
"""
import ast
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_window_cases as W            # noqa: E402
from oracle import ref_raster            # noqa: E402

SOURCE = os.path.join(ref_raster.REF_ROOT, "FlexAM", "models", "attention_utils.py")
OUT = os.path.join(ROOT, "tests", "golden", "attn_window_reference.safetensors")
L, BUILT_FOR = 70, (3, 2)                # the inputs: W.build(L, BUILT_FOR, B=1, H=2)
WINDOWS = {"causal": (-1, 0), "window_3_2": (3, 2), "window_5_open": (5, -1)}


def load_reference():
    tree = ast.parse(open(SOURCE).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "attention"]
    assert len(fns) == 1
    mod = ast.Module(body=fns, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "os": os, "warnings": warnings, "SAGE_ATTENTION_AVAILABLE": False, "FLASH_ATTN_2_AVAILABLE": False,
          "FLASH_ATTN_3_AVAILABLE": False}
    exec(compile(mod, SOURCE, "exec"), ns)
    return ns["attention"]


def main():
    from safetensors.torch import save_file
    attention = load_reference()
    q, k, v = (t.float() for t in W.build(L, BUILT_FOR, B=1, H=2))
    out = {}
    for name, window in WINDOWS.items():
        if name == "causal":
            o = attention(q, k, v, causal=True)
        else:
            o = attention(q, k, v, attn_mask=W.allowed(L, window))
        want = W.reference(q.double(), k.double(), v.double(), window, scale=W.HEAD_DIM ** -0.5)
        err = float(((o.double() - want).abs() / want.abs()).max())
        assert err <= W.FP32_REL, (name, err)                                   # the bound the CPU test holds the fixture to
        print(f"{name}: reference within {err:.2e} (relative) of the float64 restatement")
        out[name] = o.contiguous()
    save_file(out, OUT, metadata={"L": str(L), "built_for": repr(BUILT_FOR), "windows": repr(WINDOWS)})
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
