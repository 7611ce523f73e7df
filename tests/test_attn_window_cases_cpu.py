"""CPU: the windowed-attention cases of tests/attn_window_cases.py are not blind, the tile planner hip.attn_window_tiles is right, and
the float64 restatement the GPU tests compare against agrees with the reference's own attention() (tests/golden/attn_window_reference.safetensors,
written by tools/make_attn_window_golden.py from the reference's torch-SDPA branch).

Not blind: for every case, moving either bounded edge of the window by one key in either direction changes every row whose key set that
move alters by at least SENSITIVITY_ULPS bf16 ulps in some channel, and leaves every other row bit-identical.  A kernel that lets one key
too many in, or leaves one out, at any edge of any row therefore misses the 1-ulp bound of tests/test_attn_window_gpu.py.

Minimum over the altered rows, heads and moves of the largest change in ulps, as computed here:
    L600-w100_37 14, L600-w-1_0 9, L600-w0_-1 9, L600-w255_256 10, L1111-w300_0 10, L70-w3_2 105;
    L70-w80_75 has no bounded edge inside the sequence: it checks that such a window is full attention."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_window_reference.safetensors")


@pytest.mark.parametrize("case", W.CASES, ids=W.ids(W.CASES))
def test_cases_are_sensitive_to_one_key_at_either_edge(case):
    q, k, v = case.inputs()
    for t in (q, k, v):
        assert torch.equal(t.to(torch.bfloat16).double(), t)                      # the kernels get exactly these values
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    assert torch.equal(s, s.round())                                              # integer scores: every p is a power of two
    want = case.want(q, k, v)
    ok = W.allowed(case.L, case.window)
    assert bool(ok.any(1).all())                                                  # no empty row
    least = float("inf")
    for moved in W.edge_moves(case.window):
        other = W.reference(q, k, v, moved)
        altered = (W.allowed(case.L, moved) != ok).any(1)                         # [L]
        ulps = ((other - want).abs() / W.bf16_ulp(want)).amax(-1)                 # [B, L, H]: the most affected channel
        if altered.any():
            least = min(least, float(ulps[:, altered].min()))
        assert torch.equal(other[:, ~altered], want[:, ~altered]), (case.name, moved)
    print(f"{case.name}: least change of an altered row {least:.1f} ulps")
    if least < float("inf"):
        assert least >= W.SENSITIVITY_ULPS, (case.name, least)
    else:                                                                         # no edge inside the sequence: full attention
        assert bool(ok.all()) and torch.equal(want, W.reference(q, k, v, (-1, -1)))


def test_the_cases_cover_what_the_kernel_distinguishes():
    """A window narrower than a query block and one wider; a ragged L; causal and anti-causal; a window no shorter than the sequence; more
    than one batch and head; a unit whose first tiles hold no key of its last rows (the unset reference) and interior tiles."""
    spans = {c.name: c.window[0] + c.window[1] + 1 for c in W.CASES if min(c.window) >= 0}
    assert any(s < W.Q_BLOCK for s in spans.values()) and any(s > W.Q_BLOCK for s in spans.values())
    assert any(c.L % W.KV_TILE and c.L % W.Q_BLOCK for c in W.CASES)
    assert any(c.window == (-1, 0) for c in W.CASES) and any(c.window == (0, -1) for c in W.CASES)
    assert any(min(c.window) >= c.L - 1 for c in W.CASES)
    assert any(c.B >= 2 and c.H >= 3 for c in W.CASES)
    interior = False
    for c in W.CASES:
        ok = W.allowed(c.L, c.window)
        for q0 in range(0, c.L, W.Q_BLOCK):
            for t in range(-(-c.L // W.KV_TILE)):
                interior |= bool(ok[q0:q0 + W.Q_BLOCK, t * W.KV_TILE:(t + 1) * W.KV_TILE].all())
    assert interior


WINDOWS = [(100, 37), (-1, 0), (0, -1), (255, 256), (300, 0), (700, 500), (3, 2), (0, 0), (63, 0), (64, 0), (0, 63), (0, 64), (-1, -1),
           (5000, 5000), (448, 448), (-1, 200), (200, -1)]


@pytest.mark.parametrize("L", [1, 63, 64, 65, 70, 256, 257, 600, 1111, 1500])
def test_planner_equals_brute_force(L):
    from flexam_amd import hip
    assert (hip.ATTN_Q_BLOCK, hip.ATTN_KV_TILE) == (W.Q_BLOCK, W.KV_TILE)
    for window in WINDOWS:
        assert hip.attn_window_tiles(L, window) == W.tiles_brute(L, window), (L, window)


def test_planner_at_the_flagship_shape():
    """L = 11648 (26 frames of 448 tokens): +-2 frames visit under a fifth of the (query block, key tile) pairs, causal just over half."""
    from flexam_amd import hip
    L = 11648
    full = sum(b - a + 1 for a, b in hip.attn_window_tiles(L, (-1, -1)))
    assert full == 46 * 182
    share = lambda w: sum(b - a + 1 for a, b in hip.attn_window_tiles(L, w)) / full
    assert share((896, 896)) < 0.2 and 0.5 < share((-1, 0)) < 0.53
    assert hip.attn_window((5, -7)) == (5, -1) and hip.attn_window((-1, 9), causal=True) == (-1, 0)


def test_restatement_agrees_with_the_reference_attention():
    """The float64 masked softmax of tests/attn_window_cases.py against what the reference's attention() returned (is_causal=True; boolean
    attn_mask by the window rule) on the 70-token inputs in fp32, at fp32 rounding."""
    from safetensors import safe_open
    q, k, v = W.build(70, (3, 2), B=1, H=2)
    with safe_open(GOLDEN, "pt") as f:
        names = sorted(f.keys())
        assert names == ["causal", "window_3_2", "window_5_open"]
        windows = eval(f.metadata()["windows"])
        for name in names:
            ref = f.get_tensor(name)
            assert ref.dtype == torch.float32 and tuple(ref.shape) == (1, 70, 2, 128)
            want = W.reference(q, k, v, windows[name], scale=W.HEAD_DIM ** -0.5)
            err = float(((ref.double() - want).abs() / want.abs()).max())
            print(f"{name} {windows[name]}: max relative difference {err:.2e}")
            assert err <= W.FP32_REL, (name, err)
    assert windows["causal"] == (-1, 0)
    # the masks are distinct at the fixture's precision: the comparison above tells them apart
    a, b = (W.reference(q, k, v, w, scale=W.HEAD_DIM ** -0.5) for w in ((3, 2), (3, 3)))
    assert float(((a - b).abs() / a.abs()).max()) > 100 * W.FP32_REL
