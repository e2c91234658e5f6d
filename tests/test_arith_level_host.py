"""The caller-run create_proof of tests/arith_level.py over its CPU backend: the oracle's pieces, Python integers and
lookup_cases.permute_ref for every step, h from the oracle's Trace.  The bytes must be orc.create_proof's -- which pins the
DRIVER (transcript, blinding tags and indices, query order, point sets) on a machine without a GPU; the device backend
(tests/test_gpu_arith_level.py) then has only the library's entries left to be wrong about."""
import pytest

import arith_level
import poly_ref as pr
from circuits import toy_circuit


@pytest.mark.parametrize("k,two_lookups", [(5, False), (6, True)])
def test_caller_run_proof_over_the_cpu_backend_equals_the_oracle(orc, k, two_lookups):
    cs, asg, ilen = toy_circuit(k=k, two_lookups=two_lookups)
    img = cs.to_c()
    params = orc.params_new(k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    seed = 11
    st, want, tr = orc.create_proof(pk, adv, inst, seed, want_trace=True)
    assert st == 0
    h_ext = tr.array("h_ext", 1 << cs.extended_k())
    challenges = [pr.to_int(tr.fe(name)) for name in ("theta", "beta", "gamma", "y")]
    orc.trace_free(tr)
    assert arith_level.n_sets(cs) == 2 and len(cs.perm_columns) % (cs.degree() - 2), "two sets, the last not full"
    be = arith_level.HostBackend(orc, cs, fixed, sigma, params, seed, h_ext, challenges)
    got = arith_level.create_proof(be, cs, vk_repr, adv, inst)
    assert got == want
