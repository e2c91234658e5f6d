"""INTEGRATION.md section 3(a) end to end: create_proof walked by the CALLER (tests/arith_level.py) over the library's
arithmetic-level entries on device pointers -- zg_msm_batch_dev + zg_msm_finish on registered g / g_lagrange,
zg_ntt_batch_dev, zg_prover_lookup_compress_dev, zg_permute_expression_pair_dev, zg_lookup_product_terms_dev,
zg_prover_permutation_terms_dev, zg_grand_product_dev, zg_fr_random_dev, zg_prover_evaluate_h_dev,
zg_extended_to_coeff_dev, zg_eval_polys_dev, zg_fr_lincomb_dev, zg_kate_division_dev -- with every array in HBM between
the steps.  The bytes must be the oracle's create_proof's.  tests/test_arith_level_host.py holds the same driver against
the oracle over a CPU backend, so a difference here is the library's."""
import os

import numpy as np
import pytest

import arith_level
import wnn_circuit
import wnn_model
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu


def caller_run(orc, zg, ctx, cs, asg, ilen, seed, params_seed=0xABCDEF):
    """-> (the caller-run proof over the device backend, the oracle's proof, the oracle's key, the instance)"""
    k = cs.k
    img = cs.to_c()
    params = orc.params_new(k, params_seed)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    st, want, _ = orc.create_proof(pk, adv, inst, seed)
    assert st == 0
    g, gl = ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np())
    prover = zg.Prover(ctx, img, fixed, sigma, g, gl, vk_repr)
    try:
        be = arith_level.DeviceBackend(zg, ctx, prover, cs, fixed, sigma, g, gl, seed)
        got = arith_level.create_proof(be, cs, vk_repr, adv, inst)
        ctx.sync()
    finally:
        prover.close()
        g.free()
        gl.free()
    return got, want, pk, inst


def test_toy_circuit_k5_bytes_and_pairing(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(k=5)
    got, want, pk, inst = caller_run(orc, zg, ctx, cs, asg, ilen, 11)
    assert got == want
    assert orc.verify_proof_pairing(pk, inst, got) == 1


def test_two_lookups_k6(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(k=6, two_lookups=True)
    got, want, _, _ = caller_run(orc, zg, ctx, cs, asg, ilen, 12)
    assert got == want


def test_no_lookup_variant(ctx, zg, orc):
    cs, asg, ilen = variant_circuit("no_lookup")
    got, want, _, _ = caller_run(orc, zg, ctx, cs, asg, ilen, 13)
    assert got == want


def test_same_bytes_under_the_other_coset_generator(zg, orc):
    """The extended-domain arrays the caller passes between zg_prover_evaluate_h_dev and zg_extended_to_coeff_dev sit on the
    coset of the context's generator; the quotient, and so the proof, does not depend on it."""
    c1 = zg.Ctx(0)
    try:
        c1.set_coset_generator(zg.fr_cube_root(1))
        cs, asg, ilen = toy_circuit(k=5)
        got, want, _, _ = caller_run(orc, zg, c1, cs, asg, ilen, 11)
        assert got == want
    finally:
        c1.close()


def test_tiny_model_k14(ctx, zg, orc):
    """zero_g's WnnCircuit for the checked-in tiny model, one image, once."""
    kk, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), kk)
    orc.load().orc_set_threads(min(16, os.cpu_count() or 1))
    got, want, _, _ = caller_run(orc, zg, ctx, cs, asg, ilen, 7, params_seed=0x5EED)
    assert np.frombuffer(got, np.uint8).shape == np.frombuffer(want, np.uint8).shape
    assert got == want
