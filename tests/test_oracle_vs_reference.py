"""CPU: oracle vs the reference modules on cases the other fixtures do not cover (other seeds / shapes): the reference's outputs are
stored under tests/golden (oracle/make_golden.py: g4c_dit_other_shape, g7b_vae_decode_four_chunks)."""
import torch

from oracle import cases as C
from oracle import dit as O
from oracle import vae as OV


def _same_problem(fx, key, tensors):
    torch.testing.assert_close(C.checksum(tensors), fx[key], rtol=1e-9, atol=1e-9,
                               msg="seeded inputs/weights differ from the ones the fixture was generated with")


@torch.no_grad()
def test_dit_matches_reference_other_shape(golden):
    fx = golden("g4c_dit_other_shape")
    cfg = dict(O.DIT_TINY, num_layers=1)
    sd = C.dit_weights(cfg, 99)
    _same_problem(fx, "w_sum", sd)
    case = C.dit_case(cfg, 5, frames=2, h=12, w=20, batch=1, t_value=133.0)
    flat = {k: v for k, v in case.items() if torch.is_tensor(v)}
    flat.update({f"ctx{i}": u for i, u in enumerate(case["context"])})
    _same_problem(fx, "in_sum", flat)
    torch.testing.assert_close(O.dit_forward(sd, cfg, **case), fx["out"], rtol=2e-4, atol=2e-5)


@torch.no_grad()
def test_vae_decode_matches_reference_four_chunks(golden):
    fx = golden("g7b_vae_decode_four_chunks")
    vsd = C.vae_weights(C.VAE_SMALL, seed=77, prefix="")
    _same_problem(fx, "w_sum", vsd)
    z = C.vae_case(seed=78, frames=4, h=2, w=4)
    _same_problem(fx, "in_sum", dict(z=z))
    got = OV.vae_decode(vsd, z, C.VAE_SMALL["temporal_up"], OV.LATENT_MEAN, OV.LATENT_STD, prefix="")
    assert got.shape == (1, 3, 13, 32, 64)
    torch.testing.assert_close(got, fx["out"], rtol=2e-4, atol=2e-5)
