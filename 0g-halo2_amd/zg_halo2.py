"""ctypes binding of libzg_halo2.so (include/zg_halo2.h) for the Python test/bench harness.

Field elements travel as numpy ``uint64`` arrays of shape ``(..., 4)`` (little-endian limbs,
Montgomery form: the memory format of halo2curves ``bn256::Fr`` / ``Fq``), affine points as
``(..., 8)`` and Jacobian points as ``(..., 12)``.

There is no CPU fallback: ``load()`` raises if the shared library is missing and ``Ctx()`` raises
if no HIP device is visible.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_size_t, c_uint32, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZG_HALO2_LIB") or os.path.join(_HERE, "libzg_halo2.so")  # (the override is for A/B builds)

FR_MODULUS = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FQ_MODULUS = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47

_lib = None


class ZgError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"zg_halo2 status {status}: {msg}")
        self.status = status


def load() -> ctypes.CDLL:
    """Loads libzg_halo2.so; raises loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C 0g-halo2_amd` "
            "(or __graft_entry__.build()). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    lib.zg_last_error.restype = c_char_p
    lib.zg_version.restype = c_char_p
    lib.zg_ctx_stream.restype = c_void_p
    lib.zg_ctx_stream.argtypes = [c_void_p]
    lib.zg_bases_len.restype = c_size_t
    lib.zg_bases_len.argtypes = [c_void_p]
    lib.zg_bases_window_bits.restype = c_uint32
    lib.zg_bases_window_bits.argtypes = [c_void_p]
    lib.zg_ctx_destroy.argtypes = [c_void_p]
    lib.zg_ctx_destroy.restype = None
    lib.zg_bases_free.argtypes = [c_void_p]
    lib.zg_bases_free.restype = None
    lib.zg_prover_permutation_sets.restype = c_uint32
    lib.zg_prover_permutation_sets.argtypes = [c_void_p]
    lib.zg_msm_var.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_void_p]
    lib.zg_msm_var_batch.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_uint32, c_void_p]
    lib.zg_msm_var_dev.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]
    lib.zg_g1_mul_each.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.zg_g1_mul_each_dev.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.zg_g1_compress.argtypes = [c_void_p, c_size_t, c_void_p]
    lib.zg_g1_decompress.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.zg_g1_decompress_dev.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    _lib = lib
    return lib


# Every symbol include/zg_halo2.h declares (tests check the shared object exports all of them).
ABI_SYMBOLS = [
    "zg_last_error", "zg_version", "zg_ctx_create", "zg_ctx_destroy", "zg_ctx_sync", "zg_ctx_stream",
    "zg_bases_register", "zg_bases_register_dev", "zg_bases_free", "zg_bases_len",
    "zg_bases_window_bits", "zg_msm", "zg_msm_batch", "zg_msm_batch_dev", "zg_msm_finish", "zg_g1_sum",
    "zg_msm_var", "zg_msm_var_batch", "zg_msm_var_dev",
    "zg_ntt", "zg_intt", "zg_ntt_batch", "zg_intt_batch", "zg_ntt_batch_dev", "zg_coeff_to_extended",
    "zg_coeff_to_extended_batch_dev", "zg_extended_to_coeff", "zg_extended_to_coeff_dev",
    "zg_domain_omega", "zg_ctx_profile_enable", "zg_ctx_profile_collect", "zg_params_new",
    "zg_params_new_dev", "zg_prover_create", "zg_prover_destroy", "zg_prover_prove", "zg_prover_prove_dev",
    "zg_prover_proof_size", "zg_prover_fetch", "zg_grand_product_dev", "zg_eval_polys_dev",
    "zg_kate_division_dev", "zg_keccak256", "zg_ctx_profile_filter", "zg_prover_phase_ms", "zg_prover_gate_stats", "zg_ctx_trim", "zg_witness_plan_info", "zg_prover_set_overlap", "zg_ctx_set_msm_latency",
    "zg_prover_create_shared", "zg_prover_fork", "zg_prover_set_batch", "zg_prover_batch", "zg_prover_advice_slot",
    "zg_prover_prove_batch", "zg_prover_prove_batch_dev", "zg_prover_set_shard", "zg_prover_fetch_slot",
    "zg_grand_product", "zg_xyzz_sum_ranks", "zg_prover_evaluate_h",
    "zg_witness_plan_create", "zg_witness_plan_destroy", "zg_witness_plan_image_bytes", "zg_witness_plan_instance_len",
    "zg_witness_run_dev", "zg_prover_prove_images", "zg_prover_set_shard_rccl", "zg_xyzz_sum_ranks_dev", "zg_bases_enable_bit_table",
    "zg_tuning_set", "zg_tuning_get", "zg_tuning_names", "zg_bases_enable_digit_table", "zg_prover_enable_digit_tables",
    "zg_prover_vk_commitments", "zg_verifier_create", "zg_verifier_destroy", "zg_verifier_verify_batch", "zg_pairing_check",
    "zg_prover_check_batch", "zg_prover_check_batch_dev", "zg_prover_check_images", "zg_permutation_mapping",
    "zg_prover_check_circuit", "zg_prover_check_circuit_dev",
    "zg_fr_cube_root", "zg_ctx_set_coset_generator", "zg_ctx_coset_generator", "zg_prover_coset_generator",
    "zg_permutation_sigma", "zg_prover_export_key", "zg_params_lagrange", "zg_params_lagrange_dev", "zg_params_check",
    "zg_prover_proof_size_multi", "zg_prover_prove_multi", "zg_prover_prove_multi_dev", "zg_prover_prove_images_multi",
    "zg_verifier_verify_multi",
    "zg_prover_prove_circuits", "zg_prover_prove_circuits_dev", "zg_prover_prove_circuits_phased", "zg_verifier_verify_circuits",
    "zg_wnn_create", "zg_wnn_destroy", "zg_wnn_predict", "zg_wnn_predict_dev", "zg_wnn_accuracy",
    "zg_prover_evaluate_h_dev", "zg_prover_lookup_compress_dev", "zg_permute_expression_pair_dev",
    "zg_permute_expression_pair", "zg_lookup_product_terms_dev", "zg_prover_permutation_sets",
    "zg_prover_permutation_terms_dev", "zg_fr_lincomb_dev", "zg_fr_random_dev",
    "zg_prover_set_quotient_terms", "zg_prover_quotient_terms",
    "zg_g1_mul_each", "zg_g1_mul_each_dev", "zg_params_g2", "zg_g2_mul", "zg_params_update", "zg_params_update_dev",
    "zg_params_check_update",
    "zg_prover_set_multiopen", "zg_prover_multiopen", "zg_verifier_set_multiopen", "zg_verifier_multiopen",
    "zg_prover_set_transcript", "zg_prover_transcript", "zg_verifier_set_transcript", "zg_verifier_transcript",
    "zg_g1_compress", "zg_g1_decompress", "zg_g1_decompress_dev",
    "zg_prover_set_phases", "zg_prover_phases", "zg_prover_prove_phased", "zg_verifier_set_phases", "zg_verifier_phases",
    "zg_prover_create_shuffles", "zg_prover_create_shared_shuffles", "zg_prover_shuffles", "zg_verifier_create_shuffles",
    "zg_witness_plan_create_field", "zg_witness_run_field_dev", "zg_prover_prove_inputs", "zg_prover_prove_inputs_circuits",
    "zg_prover_check_inputs",
]

# zg_shuffle (include/zg_halo2.h): halo2's shuffle argument, the layout of zg_lookup
MAX_LOOKUP_WIDTH, MAX_SHUFFLES = 4, 16


class Poly(ctypes.Structure):
    _fields_ = [("first", c_uint32), ("count", c_uint32)]


class Shuffle(ctypes.Structure):
    _fields_ = [("width", c_uint32), ("inputs", Poly * MAX_LOOKUP_WIDTH), ("shuffles", Poly * MAX_LOOKUP_WIDTH)]


def shuffle_array(shuffles):
    """[(inputs [(first, count)], shuffles [(first, count)])] -> (ctypes array of zg_shuffle or None, count): ranges into the
    circuit image's monomials, to which the caller appended the expressions"""
    if not shuffles:
        return None, 0
    arr = (Shuffle * len(shuffles))()
    for j, (ins, shs) in enumerate(shuffles):
        assert len(ins) == len(shs)
        arr[j].width = len(ins)
        for e, (a, b) in enumerate(zip(ins[:MAX_LOOKUP_WIDTH], shs[:MAX_LOOKUP_WIDTH])):
            arr[j].inputs[e] = Poly(*a)
            arr[j].shuffles[e] = Poly(*b)
    return arr, len(shuffles)

# zg_query.kind of an Expression::Challenge, and the limits of zg_prover_set_phases
CHALLENGE, MAX_CHALLENGES, MAX_PHASES = 3, 16, 3
# zg_phase_fn: int fn(void *user, uint32_t phase, size_t count, const zg_fr *challenges, void *const *d_advice)
PHASE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_uint32, c_size_t, c_void_p, ctypes.POINTER(c_void_p))
_hip = None


def _hip_runtime():
    """The HIP runtime the library itself runs on (already loaded with it), for the copies of Prover.prove_phased."""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [c_void_p, c_void_p, c_size_t, c_int]
    return _hip


def _set_phases(fn, handle, n_advice, advice_phase, challenge_phase):
    adv = np.ascontiguousarray(advice_phase if advice_phase is not None else [], dtype=np.uint8)
    chal = np.ascontiguousarray(challenge_phase if challenge_phase is not None else [], dtype=np.uint8)
    if adv.size != n_advice:
        raise ValueError(f"{adv.size} advice phases for {n_advice} advice columns")
    fn.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p]
    _check(fn(handle, _ptr(adv) if adv.size else None, c_uint32(chal.size), _ptr(chal) if chal.size else None))


def _phases(fn, handle, n_advice):
    adv = np.zeros(max(n_advice, 1), np.uint8)
    chal = np.zeros(MAX_CHALLENGES, np.uint8)
    nch = c_uint32(0)
    fn.argtypes = [c_void_p, c_void_p, ctypes.POINTER(c_uint32), c_void_p]
    n = int(fn(handle, _ptr(adv), ctypes.byref(nch), _ptr(chal)))
    return n, [int(x) for x in adv[:n_advice]], [int(x) for x in chal[: nch.value]]

# zg_prover_set_multiopen / zg_verifier_set_multiopen: the multi-open argument a proof ends with
MULTIOPEN_GWC, MULTIOPEN_SHPLONK = 0, 1
# zg_prover_set_transcript / zg_verifier_set_transcript: snark-verifier's EvmTranscript (Keccak-256, uncompressed points) or
# halo2's own Blake2bWrite / Blake2bRead with Challenge255 (32-byte compressed points)
TRANSCRIPT_EVM, TRANSCRIPT_BLAKE2B = 0, 1


def g1_compress(points: np.ndarray) -> np.ndarray:
    """zg_g1_compress (host, no device): uint64[n, 8] affine points in Montgomery form -> uint8[n, 32], the GroupEncoding
    of each ((0,0) -> 32 zero bytes); no validation."""
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((points.shape[0], 32), np.uint8)
    _check(load().zg_g1_compress(_ptr(points), c_size_t(points.shape[0]), _ptr(out)))
    return out

# zg_params_check: bits of `failed`
SRS_G1_MALFORMED, SRS_G1_IDENTITY, SRS_G2, SRS_POWERS, SRS_LAGRANGE = 1, 2, 4, 8, 16
# zg_params_check_update: two more
SRS_UPDATE_BASE, SRS_UPDATE_LINK = 32, 64


def tuning_names() -> list:
    """Names of the library's tuning knobs (include/zg_halo2.h, "tuning")."""
    lib = load()
    lib.zg_tuning_names.restype = c_size_t
    n = int(lib.zg_tuning_names(None, c_size_t(0)))
    arr = (c_char_p * n)()
    lib.zg_tuning_names(arr, c_size_t(n))
    return [a.decode() for a in arr]


def tuning_set(name: str, value: int) -> None:
    """value < 0 restores the default.  Knobs that shape a proving key are read when a prover is created."""
    _check(load().zg_tuning_set(name.encode(), c_int(value)))


def tuning_get(name: str) -> int:
    v = c_int(0)
    _check(load().zg_tuning_get(name.encode(), ctypes.byref(v)))
    return v.value


EXCHANGE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_size_t, c_void_p)


def rng_key(seed) -> bytes:
    """The 32-byte blinding key of a proof: bytes pass through; an int (tests only) becomes its little-endian,
    zero-padded encoding.  Production callers pass 32 bytes from a CSPRNG (os.urandom(32))."""
    if isinstance(seed, (bytes, bytearray)):
        assert len(seed) == 32
        return bytes(seed)
    return int(seed).to_bytes(32, "little")


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", ctypes.c_uint64), ("total_ms", ctypes.c_double),
                ("algo_bytes", ctypes.c_double), ("unit_bytes", ctypes.c_double)]


FAIL_GATE, FAIL_LOOKUP, FAIL_COPY, FAIL_SHUFFLE = 0, 1, 2, 3


class Failure(ctypes.Structure):
    """zg_failure: one record of the witness check.  as_tuple(): (kind, index, row, other_index, other_row)."""
    _fields_ = [("kind", c_uint32), ("index", c_uint32), ("row", c_uint32), ("other_index", c_uint32),
                ("other_row", c_uint32)]

    def as_tuple(self) -> tuple:
        return (int(self.kind), int(self.index), int(self.row), int(self.other_index), int(self.other_row))


def permutation_mapping(sigma_values: np.ndarray, k: int):
    """zg_permutation_mapping (no device): sigma values uint64[n_perm, 2^k, 4] -> (next_col, next_row), uint32[n_perm, 2^k]
    each: sigma[c][r] = delta^next_col[c][r] * omega^next_row[c][r].  Raises ZgError when a value is no such product."""
    sigma_values = np.ascontiguousarray(sigma_values, dtype=np.uint64).reshape(-1, 1 << k, 4)
    m = sigma_values.shape[0]
    next_col = np.zeros((m, 1 << k), np.uint32)
    next_row = np.zeros((m, 1 << k), np.uint32)
    _check(load().zg_permutation_mapping(c_uint32(k), c_uint32(m), _ptr(sigma_values), _ptr(next_col), _ptr(next_row)))
    return next_col, next_row


def permutation_sigma(ctx: "Ctx", next_col: np.ndarray, next_row: np.ndarray, k: int) -> np.ndarray:
    """zg_permutation_sigma (on the device): the inverse of permutation_mapping -- (next_col, next_row), uint32[n_perm, 2^k]
    each -> sigma values uint64[n_perm, 2^k, 4], sigma[c][r] = delta^next_col[c][r] * omega^next_row[c][r].  Raises ZgError
    when an index is out of range."""
    next_col = np.ascontiguousarray(next_col, dtype=np.uint32).reshape(-1, 1 << k)
    next_row = np.ascontiguousarray(next_row, dtype=np.uint32).reshape(-1, 1 << k)
    assert next_col.shape == next_row.shape
    m = next_col.shape[0]
    sigma = np.zeros((m, 1 << k, 4), np.uint64)
    _check(ctx.lib.zg_permutation_sigma(ctx.h, c_uint32(k), c_uint32(m), _ptr(next_col), _ptr(next_row), _ptr(sigma)))
    return sigma


def fr_cube_root(which: int = 0) -> np.ndarray:
    """zg_fr_cube_root: 0 = 7^((r-1)/3), the default coset generator; 1 = its square.  Montgomery limbs."""
    out = np.zeros(4, np.uint64)
    _check(load().zg_fr_cube_root(c_uint32(which), _ptr(out)))
    return out


KEY_FIXED_POLY, KEY_SIGMA_POLY, KEY_FIXED_COSET, KEY_SIGMA_COSET, KEY_L0, KEY_L_LAST, KEY_L_ACTIVE_ROW = range(7)


def _check(status: int) -> None:
    if status != 0:
        raise ZgError(status, load().zg_last_error().decode())


def _fr(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.shape[-1] == 4, a.shape
    return a


def _ptr(a: np.ndarray) -> c_void_p:
    return c_void_p(a.ctypes.data)


def int_to_limbs(x: int) -> np.ndarray:
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def limbs_to_int(a) -> int:
    return sum(int(a[i]) << (64 * i) for i in range(4))


def fr_from_int(x: int) -> np.ndarray:
    """Canonical integer -> Montgomery limbs (host helper for tests)."""
    return int_to_limbs((x % FR_MODULUS) * (1 << 256) % FR_MODULUS)


def fr_to_int(a) -> int:
    return limbs_to_int(a) * pow(1 << 256, -1, FR_MODULUS) % FR_MODULUS


def fq_from_int(x: int) -> np.ndarray:
    return int_to_limbs((x % FQ_MODULUS) * (1 << 256) % FQ_MODULUS)


def fq_to_int(a) -> int:
    return limbs_to_int(a) * pow(1 << 256, -1, FQ_MODULUS) % FQ_MODULUS


def domain_omega(log_n: int):
    om = np.zeros(4, np.uint64)
    omi = np.zeros(4, np.uint64)
    _check(load().zg_domain_omega(c_uint32(log_n), _ptr(om), _ptr(omi)))
    return om, omi


def g1_sum(parts: np.ndarray) -> np.ndarray:
    parts = np.ascontiguousarray(parts, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, np.uint64)
    _check(load().zg_g1_sum(_ptr(parts), c_size_t(parts.shape[0]), _ptr(out)))
    return out


def pairing_check(p: np.ndarray, q: np.ndarray) -> int:
    """1 iff prod_i e(p[i], q[i]) = 1.  p: uint64[n, 8] G1 affine, q: uint64[n, 16] G2 affine (Montgomery limbs, as
    orc.Params.g2 / .s_g2 hold them); no device needed."""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8)
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 16)
    assert p.shape[0] == q.shape[0]
    res = c_int(-1)
    _check(load().zg_pairing_check(_ptr(p), _ptr(q), c_size_t(p.shape[0]), ctypes.byref(res)))
    return res.value


def params_g2(s: np.ndarray):
    """zg_params_g2: the G2 half of ParamsKZG::new -> (g2, s_g2), uint64[16] each; no device needed."""
    g2 = np.zeros(16, np.uint64)
    s_g2 = np.zeros(16, np.uint64)
    _check(load().zg_params_g2(_ptr(_fr(s)), _ptr(g2), _ptr(s_g2)))
    return g2, s_g2


def g2_mul(q: np.ndarray, t: np.ndarray) -> np.ndarray:
    """zg_g2_mul: t * q on the twist (uint64[16] G2 affine, (0,0) = identity); no device needed."""
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(16)
    out = np.zeros(16, np.uint64)
    _check(load().zg_g2_mul(_ptr(q), _ptr(_fr(t)), _ptr(out)))
    return out


def xyzz_sum_ranks(parts: np.ndarray) -> np.ndarray:
    """parts: uint64[world, count, 16] extended-Jacobian partial sums -> uint64[count, 12] normalised sums."""
    parts = np.ascontiguousarray(parts, dtype=np.uint64)
    world, count = parts.shape[0], parts.shape[1]
    out = np.zeros((count, 12), np.uint64)
    _check(load().zg_xyzz_sum_ranks(_ptr(parts), c_size_t(world), c_size_t(count), _ptr(out)))
    return out


import atexit
import weakref

_live_contexts = weakref.WeakSet()


@atexit.register
def _close_contexts_at_exit():
    # contexts (and their provers) must be torn down while the HIP runtime is still alive, not by the garbage
    # collector after the interpreter has started unloading libraries
    for c in list(_live_contexts):
        try:
            c.close()
        except Exception:  # noqa: BLE001
            pass


class Ctx:
    """One GPU (zg_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = c_void_p()
        _check(self.lib.zg_ctx_create(c_int(device), ctypes.byref(h)))
        self.h = h
        self._children = []  # weak references to the provers created on this context: they must go first
        _live_contexts.add(self)

    def _adopt(self, child):
        import weakref

        self._children.append(weakref.ref(child))

    def close(self):
        if getattr(self, "h", None):
            for ref in self._children:
                child = ref()
                if child is not None:
                    child.close()
            self._children = []
            self.lib.zg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(self.lib.zg_ctx_sync(self.h))

    def set_coset_generator(self, g_coset: np.ndarray):
        """zg_ctx_set_coset_generator: g_coset of the extended-domain transforms on this context and of the provers created
        on it from now on; one of the two fr_cube_root values, anything else raises ZgError."""
        _check(self.lib.zg_ctx_set_coset_generator(self.h, _ptr(_fr(g_coset))))

    def coset_generator(self) -> np.ndarray:
        out = np.zeros(4, np.uint64)
        _check(self.lib.zg_ctx_coset_generator(self.h, _ptr(out)))
        return out

    def drop_workspace(self) -> int:
        """zg_ctx_trim: the free blocks of the workspace pool go back to the device allocator; returns the bytes freed"""
        freed = ctypes.c_uint64(0)
        _check(self.lib.zg_ctx_trim(self.h, ctypes.byref(freed)))
        return freed.value

    @property
    def stream(self) -> int:
        return self.lib.zg_ctx_stream(self.h)

    def profile(self, on: bool):
        _check(self.lib.zg_ctx_profile_enable(self.h, c_int(1 if on else 0)))

    def profile_filter(self, kernel_name: str | None):
        _check(self.lib.zg_ctx_profile_filter(self.h, kernel_name.encode() if kernel_name else None))

    def profile_collect(self) -> dict:
        """{kernel: (launches, total_ms, algo_bytes, unit_bytes)} since the last collect; synchronises.  algo_bytes = what
        the kernel itself streams, unit_bytes = SURVEY 8d's figure of the units it carries (include/zg_halo2.h)."""
        cap = 256  # (distinct ZG_LAUNCH labels: ~60; the call drains the records, so the array must hold them all at once)
        arr = (KernelStat * cap)()
        cnt = c_size_t(0)
        _check(self.lib.zg_ctx_profile_collect(self.h, arr, c_size_t(cap), ctypes.byref(cnt)))
        if cnt.value > cap:
            raise ZgError(-1, f"zg_ctx_profile_collect: {cnt.value} kernels for an array of {cap}: records were dropped")
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms), float(arr[i].algo_bytes), float(arr[i].unit_bytes))
                for i in range(cnt.value)}

    # ---- SRS ----
    def params_new(self, k: int, s: np.ndarray):
        """ParamsKZG::new(k) with toxic scalar s -> (g, g_lagrange) as uint64[n, 8] host arrays."""
        n = 1 << k
        g = np.zeros((n, 8), np.uint64)
        gl = np.zeros((n, 8), np.uint64)
        _check(self.lib.zg_params_new(self.h, c_uint32(k), _ptr(_fr(s)), _ptr(g), _ptr(gl)))
        return g, gl

    def params_new_dev(self, k: int, s: np.ndarray, d_g: int, d_gl: int):
        _check(self.lib.zg_params_new_dev(self.h, c_uint32(k), _ptr(_fr(s)), c_void_p(d_g), c_void_p(d_gl)))

    def params_lagrange(self, k: int, g: np.ndarray) -> np.ndarray:
        """zg_params_lagrange: g_to_lagrange of the FIRST 2^k points of g (uint64[>= 2^k, 8]) -> g_lagrange uint64[2^k, 8].
        No scalar is needed; a larger SRS is downsized by passing it as it is."""
        n = 1 << k
        g = np.ascontiguousarray(np.asarray(g).reshape(-1, 8)[:n], dtype=np.uint64)
        assert g.shape[0] == n, f"{g.shape[0]} points for k = {k}"
        gl = np.zeros((n, 8), np.uint64)
        _check(self.lib.zg_params_lagrange(self.h, c_uint32(k), _ptr(g), _ptr(gl)))
        return gl

    def params_lagrange_dev(self, k: int, d_g: int, d_gl: int):
        """zg_params_lagrange_dev: device addresses (2^k * 64 B each, distinct); asynchronous on the context stream."""
        _check(self.lib.zg_params_lagrange_dev(self.h, c_uint32(k), c_void_p(d_g), c_void_p(d_gl)))

    def params_check(self, k: int, g: np.ndarray, g_lagrange, g2: np.ndarray, s_g2: np.ndarray, key):
        """zg_params_check: is (g, g_lagrange or None, g2, s_g2) a structured reference string of 2^k points?
        -> (verdict, failed): verdict 1 = accepted; failed = SRS_* bits saying why not (zg_last_error names the first
        offending point).  key: 32 bytes from a CSPRNG (an int in tests, as rng_key).  g[0] need not be the generator."""
        n = 1 << k
        g = np.ascontiguousarray(np.asarray(g).reshape(-1, 8), dtype=np.uint64)
        assert g.shape[0] == n, f"{g.shape[0]} points for k = {k}"
        gl = None
        if g_lagrange is not None:
            gl = np.ascontiguousarray(np.asarray(g_lagrange).reshape(-1, 8), dtype=np.uint64)
            assert gl.shape[0] == n, f"{gl.shape[0]} Lagrange points for k = {k}"
        g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        s_g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)
        verdict, failed = c_int(-1), c_uint32(0)
        _check(self.lib.zg_params_check(self.h, c_uint32(k), _ptr(g), _ptr(gl) if gl is not None else None, _ptr(g2),
                                        _ptr(s_g2), rng_key(key), ctypes.byref(verdict), ctypes.byref(failed)))
        return verdict.value, failed.value

    def g1_mul_each(self, points: np.ndarray, scalars: np.ndarray) -> np.ndarray:
        """zg_g1_mul_each: out[i] = scalars[i] * points[i]; points uint64[n, 8] affine, scalars uint64[n, 4] Montgomery
        -> uint64[n, 8] affine, (0,0) = identity."""
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        assert points.shape[0] == scalars.shape[0]
        out = np.zeros_like(points)
        _check(self.lib.zg_g1_mul_each(self.h, _ptr(points), _ptr(scalars), c_size_t(points.shape[0]), _ptr(out)))
        return out

    def g1_decompress(self, encodings):
        """zg_g1_decompress: GroupEncoding::from_bytes for n encodings -> (points, valid).  A host array uint8[n, 32] (or
        n * 32 bytes) gives numpy arrays uint64[n, 8] / uint8[n]; a torch tensor of n * 32 uint8 on the device gives device
        tensors int64[n, 8] / uint8[n] through zg_g1_decompress_dev (asynchronous on the context stream; the tensors are
        fenced here on both sides).  An invalid encoding: (0,0) and valid 0."""
        if hasattr(encodings, "data_ptr"):
            import torch

            enc = encodings.contiguous().view(torch.uint8).reshape(-1, 32)
            n = enc.shape[0]
            out = torch.zeros((n, 8), dtype=torch.int64, device=enc.device)
            valid = torch.zeros((n,), dtype=torch.uint8, device=enc.device)
            torch.cuda.synchronize()
            _check(self.lib.zg_g1_decompress_dev(self.h, c_void_p(enc.data_ptr() if n else 0), c_size_t(n),
                                                 c_void_p(out.data_ptr() if n else 0), c_void_p(valid.data_ptr() if n else 0)))
            self.sync()
            return out, valid
        enc = np.ascontiguousarray(np.frombuffer(encodings, np.uint8) if isinstance(encodings, (bytes, bytearray)) else encodings,
                                   dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((enc.shape[0], 8), np.uint64)
        valid = np.zeros(enc.shape[0], np.uint8)
        _check(self.lib.zg_g1_decompress(self.h, _ptr(enc), c_size_t(enc.shape[0]), _ptr(out), _ptr(valid)))
        return out, valid

    def g1_decompress_dev(self, d_in: int, n: int, d_out: int, d_valid: int):
        """zg_g1_decompress_dev: device addresses (n * 32 B in, n * 64 B and n bytes out; no aliasing); asynchronous."""
        _check(self.lib.zg_g1_decompress_dev(self.h, c_void_p(d_in), c_size_t(n), c_void_p(d_out), c_void_p(d_valid)))

    def g1_mul_each_dev(self, d_points: int, d_scalars: int, n: int, d_out: int):
        """zg_g1_mul_each_dev: device addresses (d_out may be d_points); asynchronous on the context stream."""
        _check(self.lib.zg_g1_mul_each_dev(self.h, c_void_p(d_points), c_void_p(d_scalars), c_size_t(n), c_void_p(d_out)))

    def params_update(self, k: int, t: np.ndarray, g: np.ndarray, g2: np.ndarray, s_g2: np.ndarray, lagrange: bool = True):
        """zg_params_update: one contribution t to the SRS (g, g2, s_g2) of 2^k points ->
        (g_out, g_lagrange_out or None, s_g2_out, record); record = uint64[24]: t * g[0] (8 words), t * g2 (16 words)."""
        n = 1 << k
        g = np.ascontiguousarray(np.asarray(g).reshape(-1, 8), dtype=np.uint64)
        assert g.shape[0] == n, f"{g.shape[0]} points for k = {k}"
        g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        s_g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)
        g_out = np.zeros((n, 8), np.uint64)
        gl_out = np.zeros((n, 8), np.uint64) if lagrange else None
        s_g2_out = np.zeros(16, np.uint64)
        record = np.zeros(24, np.uint64)
        _check(self.lib.zg_params_update(self.h, c_uint32(k), _ptr(_fr(t)), _ptr(g), _ptr(g2), _ptr(s_g2), _ptr(g_out),
                                         _ptr(gl_out) if lagrange else None, _ptr(s_g2_out), _ptr(record)))
        return g_out, gl_out, s_g2_out, record

    def params_update_dev(self, k: int, t: np.ndarray, d_g: int, d_g_out: int, d_gl_out: int = 0):
        """zg_params_update_dev: the G1 part on device addresses (d_g_out may be d_g; d_gl_out = 0: no Lagrange basis);
        asynchronous on the context stream."""
        _check(self.lib.zg_params_update_dev(self.h, c_uint32(k), _ptr(_fr(t)), c_void_p(d_g), c_void_p(d_g_out),
                                             c_void_p(d_gl_out) if d_gl_out else None))

    def params_check_update(self, k: int, prev_g01: np.ndarray, g_next: np.ndarray, g_lagrange_next, g2: np.ndarray,
                            s_g2_next: np.ndarray, record: np.ndarray, key):
        """zg_params_check_update: is (g_next, g_lagrange_next or None, g2, s_g2_next) the update that `record` describes of
        the SRS whose first two points are prev_g01 (uint64[2, 8])?  -> (verdict, failed); failed: SRS_* bits."""
        n = 1 << k
        prev = np.ascontiguousarray(np.asarray(prev_g01).reshape(-1, 8)[:2], dtype=np.uint64)
        assert prev.shape[0] == 2
        g = np.ascontiguousarray(np.asarray(g_next).reshape(-1, 8), dtype=np.uint64)
        assert g.shape[0] == n, f"{g.shape[0]} points for k = {k}"
        gl = None
        if g_lagrange_next is not None:
            gl = np.ascontiguousarray(np.asarray(g_lagrange_next).reshape(-1, 8), dtype=np.uint64)
            assert gl.shape[0] == n
        g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        s_g2 = np.ascontiguousarray(s_g2_next, dtype=np.uint64).reshape(16)
        record = np.ascontiguousarray(record, dtype=np.uint64).reshape(24)
        verdict, failed = c_int(-1), c_uint32(0)
        _check(self.lib.zg_params_check_update(self.h, c_uint32(k), _ptr(prev), _ptr(g), _ptr(gl) if gl is not None else None,
                                               _ptr(g2), _ptr(s_g2), _ptr(record), rng_key(key), ctypes.byref(verdict),
                                               ctypes.byref(failed)))
        return verdict.value, failed.value

    # ---- MSM ----
    def set_msm_latency(self, latency: bool):
        """True (default): two lanes per addition in the MSM reduction; False: one lane per addition."""
        _check(self.lib.zg_ctx_set_msm_latency(self.h, ctypes.c_int(1 if latency else 0)))

    def register_bases(self, bases: np.ndarray, window_bits: int = 0) -> "Bases":
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        h = c_void_p()
        _check(self.lib.zg_bases_register(self.h, _ptr(bases), c_size_t(bases.shape[0]),
                                          c_uint32(window_bits), ctypes.byref(h)))
        return Bases(self, h)

    def enable_bit_table(self, bases: "Bases", digit_width: int):
        """Bit-position table + free-position odd digits for this context's throughput-form MSMs (zg_bases_enable_bit_table)."""
        _check(self.lib.zg_bases_enable_bit_table(self.h, bases.h, c_uint32(digit_width)))

    def enable_digit_table(self, bases: "Bases", window_bits: int = 0):
        """Every multiple of every window, for lone MSMs on a latency-form context (zg_bases_enable_digit_table)."""
        _check(self.lib.zg_bases_enable_digit_table(self.h, bases.h, c_uint32(window_bits)))

    def register_bases_dev(self, d_ptr: int, n: int, window_bits: int = 0) -> "Bases":
        h = c_void_p()
        _check(self.lib.zg_bases_register_dev(self.h, c_void_p(d_ptr), c_size_t(n), c_uint32(window_bits),
                                              ctypes.byref(h)))
        return Bases(self, h)

    def msm(self, bases: "Bases", scalars: np.ndarray) -> np.ndarray:
        scalars = _fr(scalars).reshape(-1, 4)
        out = np.zeros(12, np.uint64)
        _check(self.lib.zg_msm(self.h, bases.h, _ptr(scalars), c_size_t(scalars.shape[0]), _ptr(out)))
        return out

    def msm_batch(self, bases: "Bases", scalars: np.ndarray) -> np.ndarray:
        scalars = _fr(scalars)
        assert scalars.ndim == 3
        batch, n = scalars.shape[0], scalars.shape[1]
        ptrs = (c_void_p * batch)(*[scalars[b].ctypes.data for b in range(batch)])
        out = np.zeros((batch, 12), np.uint64)
        _check(self.lib.zg_msm_batch(self.h, bases.h, ptrs, c_size_t(batch), c_size_t(n), _ptr(out)))
        return out

    def msm_batch_dev(self, bases: "Bases", d_scalars: int, stride: int, batch: int, n: int, d_out: int):
        _check(self.lib.zg_msm_batch_dev(self.h, bases.h, c_void_p(d_scalars), c_size_t(stride),
                                         c_size_t(batch), c_size_t(n), c_void_p(d_out)))

    def msm_finish(self, d_xyzz: int, batch: int) -> np.ndarray:
        out = np.zeros((batch, 12), np.uint64)
        _check(self.lib.zg_msm_finish(self.h, c_void_p(d_xyzz), c_size_t(batch), _ptr(out)))
        return out

    # ---- MSM over points that are not registered (zg_msm_var*) ----
    def msm_var(self, bases: np.ndarray, scalars: np.ndarray, window_bits: int = 0) -> np.ndarray:
        """best_multiexp(scalars, bases): bases uint64[n, 8] (any points, used once), scalars uint64[n, 4] -> normalised point."""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        scalars = _fr(scalars).reshape(-1, 4)
        assert bases.shape[0] == scalars.shape[0], f"{scalars.shape[0]} scalars for {bases.shape[0]} points"
        out = np.zeros(12, np.uint64)
        _check(self.lib.zg_msm_var(self.h, _ptr(bases), _ptr(scalars), c_size_t(scalars.shape[0]), c_uint32(window_bits), _ptr(out)))
        return out

    def msm_var_batch(self, bases: np.ndarray, scalars: np.ndarray, window_bits: int = 0) -> np.ndarray:
        """scalars uint64[batch, n, 4] against the same n points, one launch sequence -> uint64[batch, 12]."""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        scalars = _fr(scalars)
        assert scalars.ndim == 3 and scalars.shape[1] == bases.shape[0]
        batch, n = scalars.shape[0], scalars.shape[1]
        ptrs = (c_void_p * batch)(*[scalars[b].ctypes.data for b in range(batch)])
        out = np.zeros((batch, 12), np.uint64)
        _check(self.lib.zg_msm_var_batch(self.h, _ptr(bases), ptrs, c_size_t(batch), c_size_t(n), c_uint32(window_bits), _ptr(out)))
        return out

    def msm_var_dev(self, d_bases: int, d_scalars: int, stride: int, batch: int, n: int, d_out: int, window_bits: int = 0):
        """Device addresses, asynchronous on the context stream; d_out: batch x 128 B, finished by msm_finish."""
        _check(self.lib.zg_msm_var_dev(self.h, c_void_p(d_bases), c_void_p(d_scalars), c_size_t(stride), c_size_t(batch),
                                       c_size_t(n), c_uint32(window_bits), c_void_p(d_out)))

    # ---- NTT ----
    def ntt(self, a: np.ndarray, omega: np.ndarray, divisor: np.ndarray | None = None) -> np.ndarray:
        """Returns best_fft(a, omega) (times divisor when given); a is not modified."""
        a = _fr(a).reshape(-1, 4).copy()
        n = a.shape[0]
        log_n = n.bit_length() - 1
        assert 1 << log_n == n
        omega = _fr(omega)
        if divisor is None:
            _check(self.lib.zg_ntt(self.h, _ptr(a), c_uint32(log_n), _ptr(omega)))
        else:
            divisor = _fr(divisor)
            _check(self.lib.zg_intt(self.h, _ptr(a), c_uint32(log_n), _ptr(omega), _ptr(divisor)))
        return a

    def ntt_batch(self, a: np.ndarray, omega: np.ndarray, divisor: np.ndarray | None = None) -> np.ndarray:
        a = _fr(a).copy()
        assert a.ndim == 3
        batch, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        ptrs = (c_void_p * batch)(*[a[b].ctypes.data for b in range(batch)])
        omega = _fr(omega)
        if divisor is None:
            _check(self.lib.zg_ntt_batch(self.h, ptrs, c_size_t(batch), c_uint32(log_n), _ptr(omega)))
        else:
            divisor = _fr(divisor)
            _check(self.lib.zg_intt_batch(self.h, ptrs, c_size_t(batch), c_uint32(log_n), _ptr(omega),
                                          _ptr(divisor)))
        return a

    def ntt_batch_dev(self, d_a: int, stride: int, batch: int, log_n: int, omega: np.ndarray,
                      divisor: np.ndarray | None = None):
        omega = _fr(omega)
        dv = _ptr(_fr(divisor)) if divisor is not None else c_void_p(0)
        _check(self.lib.zg_ntt_batch_dev(self.h, c_void_p(d_a), c_size_t(stride), c_size_t(batch),
                                         c_uint32(log_n), _ptr(omega), dv))

    # ---- stand-alone prover building blocks (device pointers) ----
    def grand_product(self, num: np.ndarray, den: np.ndarray, z0: np.ndarray) -> np.ndarray:
        num, den = _fr(num).reshape(-1, 4), _fr(den).reshape(-1, 4)
        z = np.zeros_like(num)
        _check(self.lib.zg_grand_product(self.h, _ptr(num), _ptr(den), _ptr(_fr(z0)), c_size_t(num.shape[0]), _ptr(z)))
        return z

    def grand_product_dev(self, d_num: int, d_den: int, z0: np.ndarray, n: int, d_z: int):
        _check(self.lib.zg_grand_product_dev(self.h, c_void_p(d_num), c_void_p(d_den), _ptr(_fr(z0)), c_size_t(n),
                                             c_void_p(d_z)))

    def eval_polys_dev(self, d_polys: int, stride: int, n: int, poly_index, points: np.ndarray) -> np.ndarray:
        idx = np.ascontiguousarray(poly_index, dtype=np.uint32)
        points = _fr(points).reshape(-1, 4)
        out = np.zeros((idx.shape[0], 4), np.uint64)
        _check(self.lib.zg_eval_polys_dev(self.h, c_void_p(d_polys), c_size_t(stride), c_size_t(n),
                                          c_void_p(idx.ctypes.data), _ptr(points), c_size_t(idx.shape[0]), _ptr(out)))
        return out

    def kate_division_dev(self, d_a: int, n: int, z: np.ndarray, d_q: int):
        _check(self.lib.zg_kate_division_dev(self.h, c_void_p(d_a), c_size_t(n), _ptr(_fr(z)), c_void_p(d_q)))
        self.sync()

    # ---- the arithmetic level on device pointers ----
    def permute_expression_pair_dev(self, d_input: int, d_table: int, k: int, usable: int, d_pin: int, d_ptab: int):
        """lookup::prover::permute_expression_pair on rows < usable; zeros behind them.  Blocks (ZG_ERR_CONSTRAINT)."""
        _check(self.lib.zg_permute_expression_pair_dev(self.h, c_void_p(d_input), c_void_p(d_table), c_uint32(k),
                                                       c_uint32(usable), c_void_p(d_pin), c_void_p(d_ptab)))

    def permute_expression_pair(self, inp: np.ndarray, table: np.ndarray, usable: int):
        inp, table = _fr(inp).reshape(-1, 4), _fr(table).reshape(-1, 4)
        n = inp.shape[0]
        assert table.shape[0] == n and n == 1 << (n.bit_length() - 1)
        a, s = np.zeros_like(inp), np.zeros_like(inp)
        _check(self.lib.zg_permute_expression_pair(self.h, _ptr(inp), _ptr(table), c_uint32(n.bit_length() - 1),
                                                   c_uint32(usable), _ptr(a), _ptr(s)))
        return a, s

    def lookup_product_terms_dev(self, d_input: int, d_table: int, d_pin: int, d_ptab: int, beta, gamma, n: int,
                                 d_num: int, d_den: int):
        _check(self.lib.zg_lookup_product_terms_dev(self.h, c_void_p(d_input), c_void_p(d_table), c_void_p(d_pin),
                                                    c_void_p(d_ptab), _ptr(_fr(beta)), _ptr(_fr(gamma)), c_size_t(n),
                                                    c_void_p(d_num), c_void_p(d_den)))

    def fr_lincomb_dev(self, d_polys, coeffs, n: int, d_out: int, sub0=None):
        """d_out[i] = sum_j coeffs[j] * d_polys[j][i] (- sub0 at i = 0); d_polys: device addresses, coeffs: uint64[count, 4]."""
        count = len(d_polys)
        ptrs = (c_void_p * max(count, 1))(*[int(a) for a in d_polys])
        cf = _fr(np.asarray(coeffs, dtype=np.uint64).reshape(-1, 4)) if count else np.zeros((1, 4), np.uint64)
        assert count == 0 or cf.shape[0] == count
        _check(self.lib.zg_fr_lincomb_dev(self.h, ptrs, _ptr(cf), c_size_t(count), c_size_t(n),
                                          None if sub0 is None else _ptr(_fr(sub0)), c_void_p(d_out)))

    def fr_random_dev(self, seed, tag: int, d_out: int, count: int):
        """d_out[i] = rand_fr(key, tag, i): the blinding scalars of the prover level, under the same 32-byte key."""
        _check(self.lib.zg_fr_random_dev(self.h, rng_key(seed), c_uint32(tag), c_void_p(d_out), c_size_t(count)))

    def coeff_to_extended(self, coeffs: np.ndarray, k: int, ext_k: int) -> np.ndarray:
        coeffs = _fr(coeffs).reshape(-1, 4)
        assert coeffs.shape[0] == 1 << k
        out = np.zeros((1 << ext_k, 4), np.uint64)
        _check(self.lib.zg_coeff_to_extended(self.h, _ptr(coeffs), c_uint32(k), c_uint32(ext_k), _ptr(out)))
        return out

    def coeff_to_extended_batch_dev(self, d_in: int, in_stride: int, d_out: int, out_stride: int, batch: int,
                                    k: int, ext_k: int):
        _check(self.lib.zg_coeff_to_extended_batch_dev(self.h, c_void_p(d_in), c_size_t(in_stride),
                                                       c_void_p(d_out), c_size_t(out_stride), c_size_t(batch),
                                                       c_uint32(k), c_uint32(ext_k)))

    def extended_to_coeff(self, evals: np.ndarray, k: int, ext_k: int, out_len: int) -> np.ndarray:
        evals = _fr(evals).reshape(-1, 4).copy()
        assert evals.shape[0] == 1 << ext_k
        out = np.zeros((out_len, 4), np.uint64)
        _check(self.lib.zg_extended_to_coeff(self.h, _ptr(evals), c_uint32(k), c_uint32(ext_k),
                                             c_size_t(out_len), _ptr(out)))
        return out

    def extended_to_coeff_dev(self, d_evals: int, k: int, ext_k: int, out_len: int, d_out: int):
        _check(self.lib.zg_extended_to_coeff_dev(self.h, c_void_p(d_evals), c_uint32(k), c_uint32(ext_k),
                                                 c_size_t(out_len), c_void_p(d_out)))


def keccak256(data: bytes) -> bytes:
    out = (ctypes.c_uint8 * 32)()
    load().zg_keccak256(data, c_size_t(len(data)), out)
    return bytes(out)


class WitnessPlan:
    """zg_witness_plan: the recorded witness program of a circuit (harness/witness_tape.py WitnessProgram.arrays())
    on one context; run() writes the advice columns of a batch of inputs into device buffers."""

    def __init__(self, ctx: Ctx, arrays: dict):
        self.ctx = ctx
        lib = ctx.lib
        lib.zg_witness_plan_destroy.argtypes = [c_void_p]
        lib.zg_witness_plan_destroy.restype = None
        ops = np.ascontiguousarray(arrays["ops"], dtype=np.uint64)
        level_start = np.ascontiguousarray(arrays["level_start"], dtype=np.uint32)
        consts = np.ascontiguousarray(arrays["consts"], dtype=np.uint64)
        table = np.ascontiguousarray(arrays["table"], dtype=np.uint64)
        cell_slot = np.ascontiguousarray(arrays["cell_slot"], dtype=np.uint32)
        inst = np.ascontiguousarray(arrays["instance_slots"], dtype=np.uint32)
        self.n_advice, n = cell_slot.shape
        self.k = n.bit_length() - 1
        self.n_instance = int(inst.shape[0])
        self.image_bytes = int(arrays["image_bytes"])
        h = c_void_p()
        args = [ctx.h, _ptr(ops), c_size_t(ops.shape[0]), _ptr(level_start), c_size_t(level_start.shape[0] - 1), _ptr(consts),
                c_size_t(consts.shape[0]), _ptr(table), c_size_t(table.shape[0]), _ptr(cell_slot), c_uint32(self.n_advice),
                c_uint32(self.k), _ptr(inst), c_size_t(self.n_instance), c_size_t(self.image_bytes)]
        self.n_challenges = 0
        if "phase_level_start" in arrays:
            # zg_witness_plan_create_field: field operations, challenges, advice phases
            pls = np.ascontiguousarray(arrays["phase_level_start"], dtype=np.uint32)
            adv = np.ascontiguousarray(arrays["advice_phase"], dtype=np.uint8)
            chal = np.ascontiguousarray(arrays.get("challenge_phase", []), dtype=np.uint8)
            if adv.size != self.n_advice:
                raise ValueError(f"{adv.size} advice phases for {self.n_advice} advice columns")
            self.n_challenges = int(chal.size)
            _check(lib.zg_witness_plan_create_field(*args, _ptr(pls), c_uint32(pls.size - 1), _ptr(adv), c_uint32(chal.size),
                                                    _ptr(chal) if chal.size else None, ctypes.byref(h)))
        else:
            _check(lib.zg_witness_plan_create(*args, ctypes.byref(h)))
        self.h = h
        ctx._adopt(self)

    def info(self) -> dict:
        """zg_witness_plan_info: how the program was laid out (LDS cells, values left in HBM, levels with a global barrier)"""
        out = (ctypes.c_uint64 * 10)()
        _check(self.ctx.lib.zg_witness_plan_info(self.h, out, c_size_t(10)))
        return dict(zip(("lds_bytes", "narrow_cells", "wide_cells", "values_in_lds", "values_in_hbm", "hbm_levels", "wide_values", "levels",
                         "narrow_ops", "lanes"),
                        (int(x) for x in out)))

    def run(self, images: np.ndarray, d_advice) -> np.ndarray:
        """images: uint8[count, image_bytes...]; d_advice: `count` device addresses ([n_advice][2^k] field elements
        each).  Returns the instance values, uint64[count, n_instance, 4] (Montgomery form)."""
        images = np.ascontiguousarray(images, dtype=np.uint8).reshape(len(d_advice), -1)
        assert images.shape[1] == self.image_bytes, "image size does not match the recorded program"
        count = images.shape[0]
        ptrs = (c_void_p * count)(*[c_void_p(a) for a in d_advice])
        out = np.zeros((count, self.n_instance, 4), np.uint64)
        _check(self.ctx.lib.zg_witness_run_dev(self.h, _ptr(images), c_size_t(count), ptrs, _ptr(out)))
        return out

    def run_field(self, inputs: np.ndarray, d_advice, challenges=None) -> np.ndarray:
        """zg_witness_run_field_dev: run() for a plan with challenges -- every phase for the caller's challenge values,
        uint64[count, n_challenges, 4] (Montgomery limbs; None for a plan without challenges).  Returns the instance values."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8).reshape(len(d_advice), -1)
        assert inputs.shape[1] == self.image_bytes, "input size does not match the recorded program"
        count = inputs.shape[0]
        chal = None
        if challenges is not None:
            chal = np.ascontiguousarray(challenges, dtype=np.uint64)
            if chal.shape != (count, self.n_challenges, 4):
                raise ValueError(f"challenges of shape {chal.shape} for {count} inputs of {self.n_challenges} challenges")
        ptrs = (c_void_p * count)(*[c_void_p(a) for a in d_advice])
        out = np.zeros((count, self.n_instance, 4), np.uint64)
        _check(self.ctx.lib.zg_witness_run_field_dev(self.h, _ptr(inputs), c_size_t(count), _ptr(chal) if chal is not None and chal.size else None,
                                                     ptrs, _ptr(out)))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.zg_witness_plan_destroy(self.h)
            self.h = None


class Prover:
    """zg_prover: create_proof for one circuit (circuit.py CircuitImage) on one GPU, one proof or a lock-step batch."""

    def __init__(self, ctx: Ctx, image, fixed_values: np.ndarray = None, sigma_values: np.ndarray = None, g=None,
                 g_lagrange=None, vk_repr: np.ndarray = None, _handle=None, _keep=None, shuffles=None):
        """g / g_lagrange: uint64[n, 8] host arrays, or two `Bases` handles shared between provers.
        shuffles: the circuit's shuffle arguments (shuffle_array's input, or a (ctypes array, count) pair):
        zg_prover_create_shuffles / zg_prover_create_shared_shuffles."""
        self.ctx = ctx
        self.image = image
        lib = ctx.lib
        lib.zg_prover_proof_size.restype = c_size_t
        lib.zg_prover_proof_size.argtypes = [c_void_p]
        lib.zg_prover_destroy.argtypes = [c_void_p]
        lib.zg_prover_destroy.restype = None
        lib.zg_prover_batch.restype = c_size_t
        lib.zg_prover_batch.argtypes = [c_void_p]
        lib.zg_prover_advice_slot.restype = c_void_p
        lib.zg_prover_advice_slot.argtypes = [c_void_p, c_size_t]
        self._keep = _keep  # (a fork holds its parent: the parent's exchange trampolines outlive every fork)
        self._exchange = None
        # every exchange trampoline this prover was ever given: zg_prover_fork copies the raw function pointer into the
        # fork on the C side, so a superseded callback must stay alive for as long as a fork may still call it
        self._exchanges = [] if _keep is None else _keep._exchanges
        if _handle is not None:
            h = _handle
        else:
            fixed_values = np.ascontiguousarray(fixed_values, dtype=np.uint64)
            sigma_values = np.ascontiguousarray(sigma_values, dtype=np.uint64)
            h = c_void_p()
            sh = shuffles if isinstance(shuffles, tuple) else shuffle_array(shuffles) if shuffles is not None else None
            if isinstance(g, Bases):
                self._bases = (g, g_lagrange)  # keep the shared tables alive
                if sh is not None:
                    _check(lib.zg_prover_create_shared_shuffles(ctx.h, image.ptr(), sh[0], c_uint32(sh[1]), _ptr(fixed_values),
                                                                _ptr(sigma_values), g.h, g_lagrange.h, _ptr(_fr(vk_repr)),
                                                                ctypes.byref(h)))
                else:
                    _check(lib.zg_prover_create_shared(ctx.h, image.ptr(), _ptr(fixed_values), _ptr(sigma_values), g.h,
                                                       g_lagrange.h, _ptr(_fr(vk_repr)), ctypes.byref(h)))
            else:
                g = np.ascontiguousarray(g, dtype=np.uint64)
                g_lagrange = np.ascontiguousarray(g_lagrange, dtype=np.uint64)
                if sh is not None:
                    _check(lib.zg_prover_create_shuffles(ctx.h, image.ptr(), sh[0], c_uint32(sh[1]), _ptr(fixed_values),
                                                         _ptr(sigma_values), _ptr(g), _ptr(g_lagrange), _ptr(_fr(vk_repr)),
                                                         ctypes.byref(h)))
                else:
                    _check(lib.zg_prover_create(ctx.h, image.ptr(), _ptr(fixed_values), _ptr(sigma_values), _ptr(g),
                                                _ptr(g_lagrange), _ptr(_fr(vk_repr)), ctypes.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.n = 1 << image.c.k
        self.n_advice = image.c.n_advice
        self.proof_cap = int(lib.zg_prover_proof_size(h))

    @property
    def shuffles(self) -> int:
        """zg_prover_shuffles: the number of shuffle arguments of the prover's circuit"""
        self.ctx.lib.zg_prover_shuffles.argtypes = [c_void_p]
        self.ctx.lib.zg_prover_shuffles.restype = c_uint32
        return int(self.ctx.lib.zg_prover_shuffles(self.h))

    def fork(self, ctx: Ctx) -> "Prover":
        """Another prover on the same proving key and base tables (no copy), on another context of the device."""
        h = c_void_p()
        _check(self.ctx.lib.zg_prover_fork(self.h, ctx.h, ctypes.byref(h)))
        return Prover(ctx, self.image, _handle=h, _keep=self)

    def set_batch(self, max_batch: int):
        _check(self.ctx.lib.zg_prover_set_batch(self.h, c_size_t(max_batch)))

    def set_multiopen(self, scheme: int):
        """zg_prover_set_multiopen: MULTIOPEN_GWC (default) or MULTIOPEN_SHPLONK; the size bounds follow it."""
        self.ctx.lib.zg_prover_set_multiopen.argtypes = [c_void_p, ctypes.c_int]
        _check(self.ctx.lib.zg_prover_set_multiopen(self.h, ctypes.c_int(scheme)))
        self.proof_cap = int(self.ctx.lib.zg_prover_proof_size(self.h))

    @property
    def multiopen(self) -> int:
        self.ctx.lib.zg_prover_multiopen.argtypes = [c_void_p]
        return int(self.ctx.lib.zg_prover_multiopen(self.h))

    def set_transcript(self, transcript: int):
        """zg_prover_set_transcript: TRANSCRIPT_EVM (default) or TRANSCRIPT_BLAKE2B; the size bounds follow it."""
        self.ctx.lib.zg_prover_set_transcript.argtypes = [c_void_p, ctypes.c_int]
        _check(self.ctx.lib.zg_prover_set_transcript(self.h, ctypes.c_int(transcript)))
        self.proof_cap = int(self.ctx.lib.zg_prover_proof_size(self.h))

    @property
    def transcript(self) -> int:
        self.ctx.lib.zg_prover_transcript.argtypes = [c_void_p]
        return int(self.ctx.lib.zg_prover_transcript(self.h))

    def set_phases(self, advice_phase, challenge_phase):
        """zg_prover_set_phases: the phase of every advice column and of every challenge squeezed (lists of small ints)."""
        _set_phases(self.ctx.lib.zg_prover_set_phases, self.h, self.n_advice, advice_phase, challenge_phase)

    @property
    def phases(self):
        """zg_prover_phases: (number of phases, advice phases, challenge phases)."""
        return _phases(self.ctx.lib.zg_prover_phases, self.h, self.n_advice)

    def prove_phased_c(self, fn_ptr, instances, seeds, user: int = 0, raise_on_error=True):
        """zg_prover_prove_phased with a zg_phase_fn given as a PHASE_FN object or the address of a C function."""
        count = len(seeds)
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = self._inst(instances[b])
            insts.append(i)
        inst_ptrs = (c_void_p * count)(*[c_void_p(i.ctypes.data) for i in insts])
        keys = b"".join(rng_key(s) for s in seeds)
        bufs = [(ctypes.c_uint8 * self.proof_cap)() for _ in range(count)]
        out_ptrs = (c_void_p * count)(*[ctypes.addressof(b) for b in bufs])
        lens = (c_size_t * count)()
        fn = fn_ptr if isinstance(fn_ptr, PHASE_FN) else ctypes.cast(fn_ptr, PHASE_FN)
        lib = self.ctx.lib
        lib.zg_prover_prove_phased.argtypes = [c_void_p, c_size_t, PHASE_FN, c_void_p, c_void_p, c_size_t, ctypes.c_char_p, c_void_p, c_void_p]
        st = lib.zg_prover_prove_phased(self.h, c_size_t(count), fn, c_void_p(user), inst_ptrs, c_size_t(inst_len), keys, out_ptrs, lens)
        if st != 0 and raise_on_error:
            _check(st)
        return [bytes(bufs[b][: lens[b]]) for b in range(count)], st

    def prove_phased(self, synthesize, instances, seeds, raise_on_error=True):
        """zg_prover_prove_phased with the witness made by a Python function: synthesize(phase, challenges) is called once
        per phase with challenges uint64[count, n_challenges, 4] (Montgomery limbs, zero where not yet squeezed) and returns,
        per proof, a dict {advice column: uint64[rows, 4]} of the columns of that phase, rows >= the usable rows; their
        usable rows are copied into the proof's slot before the call returns to the library (the blinding rows are the
        library's).  An exception, or a column outside 0 .. n_advice, aborts the batch (status -1).  Returns (proofs, status)."""
        return self.prove_phased_c(self._phase_callback(synthesize), instances, seeds, raise_on_error=raise_on_error)

    def _phase_callback(self, synthesize):
        """the zg_phase_fn of prove_phased / prove_circuits_phased around a Python `synthesize`"""
        n, hip = self.n, _hip_runtime()
        usable = n - (self.image.c.blinding_factors + 1)
        nch = len(self.phases[2])

        def _cb(_user, phase, cnt, challenges, d_advice):
            try:
                ch = np.zeros((cnt, nch, 4), np.uint64)
                if nch:
                    ctypes.memmove(ch.ctypes.data, challenges, ch.nbytes)
                cols = synthesize(int(phase), ch)
                for b in range(cnt):
                    for col, values in cols[b].items():
                        if not 0 <= int(col) < self.n_advice:
                            return 2
                        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)[:usable]
                        if v.shape[0] != usable:
                            return 3
                        if hip.hipMemcpy(c_void_p(d_advice[b] + int(col) * n * 32), c_void_p(v.ctypes.data), c_size_t(v.nbytes), 1) != 0:
                            return 4
                return 0
            except Exception:  # noqa: BLE001 -- nothing may propagate through the C frames
                import traceback

                traceback.print_exc()
                return 1

        return PHASE_FN(_cb)

    @property
    def batch(self) -> int:
        return int(self.ctx.lib.zg_prover_batch(self.h))

    def advice_slot(self, slot: int) -> int:
        """Device address of the advice columns of proof slot `slot` ([n_advice][2^k] field elements)."""
        return int(self.ctx.lib.zg_prover_advice_slot(self.h, c_size_t(slot)))

    def set_shard(self, rank: int, world: int, first_point: int, exchange):
        """exchange(send: bytes-like view, recv: writable view of world * len(send) bytes) = all-gather."""
        def _cb(_user, send, nbytes, recv):
            try:
                src = (ctypes.c_uint8 * nbytes).from_address(send)
                dst = (ctypes.c_uint8 * (nbytes * world)).from_address(recv)
                exchange(src, dst)
                return 0
            except Exception:  # noqa: BLE001 -- nothing may propagate through the C frames
                import traceback

                traceback.print_exc()
                return 1

        self._exchange = EXCHANGE_FN(_cb) if world > 1 else None
        if self._exchange is not None:
            self._exchanges.append(self._exchange)
        fn = self._exchange if self._exchange is not None else ctypes.cast(None, EXCHANGE_FN)
        _check(self.ctx.lib.zg_prover_set_shard(self.h, c_uint32(rank), c_uint32(world), c_size_t(first_point), fn, None))

    def set_shard_c(self, rank: int, world: int, first_point: int, fn_ptr: int, user: int = 0):
        """zg_prover_set_shard with a C function as the exchange (address of an
        `int fn(void *user, const void *send, size_t nbytes, void *recv)`): no Python in the provers' threads."""
        _check(self.ctx.lib.zg_prover_set_shard(self.h, c_uint32(rank), c_uint32(world), c_size_t(first_point),
                                                ctypes.cast(fn_ptr, EXCHANGE_FN), c_void_p(user)))

    def set_shard_rccl(self, rank: int, world: int, first_point: int, comm: int):
        """comm: an initialised ncclComm_t (multi_gpu.RcclComm(...).handle); the exchange then runs inside the library."""
        _check(self.ctx.lib.zg_prover_set_shard_rccl(self.h, c_uint32(rank), c_uint32(world), c_size_t(first_point),
                                                     c_void_p(comm)))

    @staticmethod
    def _inst(instance):
        instance = np.ascontiguousarray(instance, dtype=np.uint64)
        inst_len = instance.shape[1] if instance.ndim == 3 and instance.shape[0] else 0
        return instance, inst_len

    def prove(self, advice: np.ndarray, instance: np.ndarray, seed) -> bytes:
        advice = np.ascontiguousarray(advice, dtype=np.uint64)
        instance, inst_len = self._inst(instance)
        buf = (ctypes.c_uint8 * self.proof_cap)()
        plen = c_size_t(0)
        _check(self.ctx.lib.zg_prover_prove(self.h, _ptr(advice), _ptr(instance), c_size_t(inst_len), rng_key(seed), buf,
                                            c_size_t(self.proof_cap), ctypes.byref(plen)))
        return bytes(buf[: plen.value])

    def prove_dev(self, d_advice: int, instance: np.ndarray, seed) -> bytes:
        instance, inst_len = self._inst(instance)
        buf = (ctypes.c_uint8 * self.proof_cap)()
        plen = c_size_t(0)
        _check(self.ctx.lib.zg_prover_prove_dev(self.h, c_void_p(d_advice), _ptr(instance), c_size_t(inst_len),
                                                rng_key(seed), buf, c_size_t(self.proof_cap), ctypes.byref(plen)))
        return bytes(buf[: plen.value])

    def prove_batch(self, advice, instances, seeds, device=False, raise_on_error=True):
        """count = len(seeds) proofs in lock step.  advice: list of host arrays (device=False) or device addresses
        (device=True); None entries (or advice=None) = the slot already holds the columns.  Returns (proofs, statuses)."""
        count = len(seeds)
        lib = self.ctx.lib
        keep = []
        if advice is None:
            adv_ptrs = None
        elif device:
            adv_ptrs = (c_void_p * count)(*[c_void_p(a) if a else None for a in advice])
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint64) if a is not None else None for a in advice]
            adv_ptrs = (c_void_p * count)(*[c_void_p(a.ctypes.data) if a is not None else None for a in keep])
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = self._inst(instances[b])
            insts.append(i)
        inst_ptrs = (c_void_p * count)(*[c_void_p(i.ctypes.data) for i in insts])
        keys = b"".join(rng_key(s) for s in seeds)
        bufs = [(ctypes.c_uint8 * self.proof_cap)() for _ in range(count)]
        out_ptrs = (c_void_p * count)(*[ctypes.addressof(b) for b in bufs])
        lens = (c_size_t * count)()
        sts = (c_int * count)()
        fn = lib.zg_prover_prove_batch_dev if device else lib.zg_prover_prove_batch
        st = fn(self.h, c_size_t(count), adv_ptrs, inst_ptrs, c_size_t(inst_len), keys, out_ptrs,
                c_size_t(self.proof_cap), lens, sts)
        if st != 0 and raise_on_error:
            _check(st)
        return [bytes(bufs[b][: lens[b]]) for b in range(count)], list(sts)

    def prove_images(self, plan: "WitnessPlan", images: np.ndarray, seeds, raise_on_error=True):
        """Wnn::proof for a batch: image bytes -> (proofs, outputs uint64[count, n_instance, 4], statuses)."""
        count = len(seeds)
        images = np.ascontiguousarray(images, dtype=np.uint8).reshape(count, -1)
        keys = b"".join(rng_key(s) for s in seeds)
        bufs = [(ctypes.c_uint8 * self.proof_cap)() for _ in range(count)]
        out_ptrs = (c_void_p * count)(*[ctypes.addressof(b) for b in bufs])
        lens = (c_size_t * count)()
        sts = (c_int * count)()
        outputs = np.zeros((count, plan.n_instance, 4), np.uint64)
        st = self.ctx.lib.zg_prover_prove_images(self.h, plan.h, _ptr(images), c_size_t(count), keys, out_ptrs,
                                                 c_size_t(self.proof_cap), lens, _ptr(outputs), sts)
        if st != 0 and raise_on_error:
            _check(st)
        return [bytes(bufs[b][: lens[b]]) for b in range(count)], outputs, list(sts)

    def prove_inputs(self, plan: "WitnessPlan", inputs: np.ndarray, seeds, raise_on_error=True):
        """zg_prover_prove_inputs: prove_images for every circuit the library proves -- input bytes -> (proofs, outputs
        uint64[count, n_instance, 4], statuses); a circuit with advice phases has its later phases replayed by the plan
        with the challenges the proof squeezes.  The plan's phases must be the prover's."""
        count = len(seeds)
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8).reshape(count, -1)
        keys = b"".join(rng_key(s) for s in seeds)
        bufs = [(ctypes.c_uint8 * self.proof_cap)() for _ in range(count)]
        out_ptrs = (c_void_p * count)(*[ctypes.addressof(b) for b in bufs])
        lens = (c_size_t * count)()
        sts = (c_int * count)()
        outputs = np.zeros((count, plan.n_instance, 4), np.uint64)
        st = self.ctx.lib.zg_prover_prove_inputs(self.h, plan.h, _ptr(inputs), c_size_t(count), keys, out_ptrs,
                                                 c_size_t(self.proof_cap), lens, _ptr(outputs), sts)
        if st != 0 and raise_on_error:
            _check(st)
        return [bytes(bufs[b][: lens[b]]) for b in range(count)], outputs, list(sts)

    def prove_inputs_circuits(self, plan: "WitnessPlan", inputs: np.ndarray, seeds):
        """zg_prover_prove_inputs_circuits: len(seeds) inputs in ONE proof (prove_circuits / prove_circuits_phased with the
        plan as the witness): input bytes -> (proof, outputs uint64[circuits, n_instance, 4])."""
        count = len(seeds)
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8).reshape(max(count, 1), -1)
        keys = b"".join(rng_key(s) for s in seeds)
        cap = max(self.proof_size_multi(count), 1)
        buf = (ctypes.c_uint8 * cap)()
        plen = c_size_t(0)
        outputs = np.zeros((max(count, 1), plan.n_instance, 4), np.uint64)
        _check(self.ctx.lib.zg_prover_prove_inputs_circuits(self.h, plan.h, _ptr(inputs), c_size_t(count), keys, buf, c_size_t(cap),
                                                            ctypes.byref(plen), _ptr(outputs)))
        return bytes(buf[: plen.value]), outputs

    def check_inputs(self, plan: "WitnessPlan", inputs: np.ndarray, challenges=None, cap: int = 64):
        """zg_prover_check_inputs: input bytes -> (reports as check_circuit, outputs uint64[count, n_instance, 4]); the
        witness is the plan's for the caller's challenges, uint64[count, n_challenges, 4] (None without challenges)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8)
        count = inputs.shape[0]
        inputs = inputs.reshape(count, -1)
        chal = None
        if challenges is not None:
            chal = np.ascontiguousarray(challenges, dtype=np.uint64)
            if chal.shape != (count, plan.n_challenges, 4):
                raise ValueError(f"challenges of shape {chal.shape} for {count} inputs of {plan.n_challenges} challenges")
        outputs = np.zeros((count, plan.n_instance, 4), np.uint64)
        recs = (Failure * max(1, count * cap))()
        totals = (c_uint32 * (4 * count))()
        _check(self.ctx.lib.zg_prover_check_inputs(self.h, plan.h, _ptr(inputs), c_size_t(count),
                                                   _ptr(chal) if chal is not None and chal.size else None, _ptr(outputs),
                                                   recs if cap else None, c_size_t(cap), totals))
        return self._reports(count, cap, recs, totals, 4), outputs

    # ---- one proof of several circuit instances (create_proof's `circuits` slice)
    def proof_size_multi(self, circuits: int) -> int:
        """zg_prover_proof_size_multi: upper bound of the size of a proof of `circuits` instances, bytes."""
        fn = self.ctx.lib.zg_prover_proof_size_multi
        fn.restype = c_size_t
        fn.argtypes = [c_void_p, c_size_t]
        return int(fn(self.h, circuits))

    def prove_multi(self, advice, instances, seeds, device=False) -> bytes:
        """ONE proof of len(seeds) circuit instances (<= the prover's batch): one transcript, one h, one GWC opening.
        advice / instances / seeds per circuit, as prove_batch takes them (device=True: zg_prover_prove_multi_dev).
        A lookup failure in any circuit raises ZgError(ZG_ERR_CONSTRAINT)."""
        lib = self.ctx.lib
        return self._prove_one(lib.zg_prover_prove_multi_dev if device else lib.zg_prover_prove_multi, advice, instances, seeds, device)

    def _prove_one(self, fn, advice, instances, seeds, device) -> bytes:
        """the call of zg_prover_prove_multi* / zg_prover_prove_circuits*: one proof of len(seeds) circuits"""
        count = len(seeds)
        keep = []
        if advice is None:
            adv_ptrs = None
        elif device:
            adv_ptrs = (c_void_p * count)(*[c_void_p(a) if a else None for a in advice])
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint64) if a is not None else None for a in advice]
            adv_ptrs = (c_void_p * count)(*[c_void_p(a.ctypes.data) if a is not None else None for a in keep])
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = self._inst(instances[b])
            insts.append(i)
        inst_ptrs = (c_void_p * max(count, 1))(*[c_void_p(i.ctypes.data) for i in insts])
        keys = b"".join(rng_key(s) for s in seeds)
        cap = max(self.proof_size_multi(count), 1)
        buf = (ctypes.c_uint8 * cap)()
        plen = c_size_t(0)
        _check(fn(self.h, c_size_t(count), adv_ptrs, inst_ptrs, c_size_t(inst_len), keys, buf, c_size_t(cap), ctypes.byref(plen)))
        return bytes(buf[: plen.value])

    def prove_circuits(self, advice, instances, seeds, device=False) -> bytes:
        """zg_prover_prove_circuits / _dev: prove_multi for every circuit the library proves -- shuffles, challenges (every
        advice column in phase 0) and, through prove_circuits_phased, advice phases.  The same arguments."""
        lib = self.ctx.lib
        return self._prove_one(lib.zg_prover_prove_circuits_dev if device else lib.zg_prover_prove_circuits, advice, instances, seeds, device)

    def prove_circuits_phased_c(self, fn_ptr, instances, seeds, user: int = 0, raise_on_error=True):
        """zg_prover_prove_circuits_phased with a zg_phase_fn given as a PHASE_FN object or the address of a C function."""
        count = len(seeds)
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = self._inst(instances[b])
            insts.append(i)
        inst_ptrs = (c_void_p * max(count, 1))(*[c_void_p(i.ctypes.data) for i in insts])
        keys = b"".join(rng_key(s) for s in seeds)
        cap = max(self.proof_size_multi(count), 1)
        buf = (ctypes.c_uint8 * cap)()
        plen = c_size_t(0)
        fn = fn_ptr if isinstance(fn_ptr, PHASE_FN) else ctypes.cast(fn_ptr, PHASE_FN)
        call = self.ctx.lib.zg_prover_prove_circuits_phased
        call.argtypes = [c_void_p, c_size_t, PHASE_FN, c_void_p, c_void_p, c_size_t, ctypes.c_char_p, c_void_p, c_size_t, c_void_p]
        st = call(self.h, c_size_t(count), fn, c_void_p(user), inst_ptrs, c_size_t(inst_len), keys, buf, c_size_t(cap), ctypes.byref(plen))
        if st != 0 and raise_on_error:
            _check(st)
        return bytes(buf[: plen.value]), st

    def prove_circuits_phased(self, synthesize, instances, seeds, raise_on_error=True):
        """zg_prover_prove_circuits_phased with the witness made by a Python function, prove_phased's convention:
        synthesize(phase, challenges) is called once per phase with challenges uint64[circuits, n_challenges, 4] -- every row
        the same values, the proof has one transcript -- and returns, per circuit, a dict {advice column: uint64[rows, 4]}.
        Returns (proof, status); an exception in the callback gives (b"", -1)."""
        return self.prove_circuits_phased_c(self._phase_callback(synthesize), instances, seeds, raise_on_error=raise_on_error)

    def prove_multi_dev(self, d_advice, instances, seeds) -> bytes:
        """prove_multi with the advice columns in HBM (device addresses, or None = the slots as they stand)."""
        return self.prove_multi(d_advice, instances, seeds, device=True)

    def prove_images_multi(self, plan: "WitnessPlan", images: np.ndarray, seeds):
        """Wnn::proof for len(seeds) images in ONE proof: image bytes -> (proof, outputs uint64[circuits, n_instance, 4])."""
        count = len(seeds)
        images = np.ascontiguousarray(images, dtype=np.uint8).reshape(max(count, 1), -1)
        keys = b"".join(rng_key(s) for s in seeds)
        cap = max(self.proof_size_multi(count), 1)
        buf = (ctypes.c_uint8 * cap)()
        plen = c_size_t(0)
        outputs = np.zeros((max(count, 1), plan.n_instance, 4), np.uint64)
        _check(self.ctx.lib.zg_prover_prove_images_multi(self.h, plan.h, _ptr(images), c_size_t(count), keys, buf, c_size_t(cap),
                                                         ctypes.byref(plen), _ptr(outputs)))
        return bytes(buf[: plen.value]), outputs

    # ---- witness check (Wnn::mock_proof)
    @staticmethod
    def _reports(count, cap, recs, totals, kinds=3):
        out = []
        for b in range(count):
            t = [int(totals[kinds * b + j]) for j in range(kinds)]
            out.append((t, [recs[b * cap + i].as_tuple() for i in range(min(sum(t), cap))]))
        return out

    def check_batch(self, advice, instances, cap: int = 64, device: bool = False):
        """zg_prover_check_batch(_dev): one (totals, records) per witness -- totals = [gate, lookup, copy] failure counts,
        records = the first min(sum(totals), cap) failures as (kind, index, row, other_index, other_row), ascending.
        advice: list of host arrays (device=False) or device addresses (device=True); None entries (or advice=None) =
        the slot as it stands.  The slots are only read."""
        count = len(instances)
        lib = self.ctx.lib
        keep = []
        if advice is None:
            adv_ptrs = None
        elif device:
            adv_ptrs = (c_void_p * count)(*[c_void_p(a) if a else None for a in advice])
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint64) if a is not None else None for a in advice]
            adv_ptrs = (c_void_p * count)(*[c_void_p(a.ctypes.data) if a is not None else None for a in keep])
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = self._inst(instances[b])
            insts.append(i)
        inst_ptrs = (c_void_p * count)(*[c_void_p(i.ctypes.data) for i in insts])
        recs = (Failure * max(1, count * cap))()
        totals = (c_uint32 * (3 * count))()
        fn = lib.zg_prover_check_batch_dev if device else lib.zg_prover_check_batch
        _check(fn(self.h, c_size_t(count), adv_ptrs, inst_ptrs, c_size_t(inst_len), recs if cap else None, c_size_t(cap),
                  totals))
        return self._reports(count, cap, recs, totals)

    def check(self, advice: np.ndarray, instance: np.ndarray, cap: int = 64):
        """One witness: (totals, records); see check_batch."""
        return self.check_batch([advice], [instance], cap)[0]

    @property
    def n_challenges(self) -> int:
        """The challenges per witness zg_prover_check_circuit expects: zg_prover_phases' count, or (no phases set) the
        circuit's own, 1 + the largest index a challenge query names."""
        nch = len(self.phases[2])
        if nch:
            return nch
        c = self.image.c
        return max([c.queries[i].column + 1 for i in range(c.n_queries) if c.queries[i].kind == 3], default=0)

    def check_circuit(self, advice, instances, challenges=None, cap: int = 64, device: bool = False):
        """zg_prover_check_circuit(_dev): the witness check for a circuit with shuffles and challenges.  One (totals,
        records) per witness as check_batch, totals = [gate, lookup, copy, shuffle]; a shuffle record is (3, shuffle, input
        row, 0, the shuffle row it met).  challenges: uint64[count, n_challenges, 4], the caller's values (Montgomery limbs),
        None for a circuit without challenges; the witness is whole, synthesised for those values."""
        count = len(instances)
        lib = self.ctx.lib
        keep = []
        if advice is None:
            adv_ptrs = None
        elif device:
            adv_ptrs = (c_void_p * count)(*[c_void_p(a) if a else None for a in advice])
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint64) if a is not None else None for a in advice]
            adv_ptrs = (c_void_p * count)(*[c_void_p(a.ctypes.data) if a is not None else None for a in keep])
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = self._inst(instances[b])
            insts.append(i)
        inst_ptrs = (c_void_p * count)(*[c_void_p(i.ctypes.data) for i in insts])
        chal = None
        if challenges is not None:
            chal = np.ascontiguousarray(challenges, dtype=np.uint64)
            if chal.shape != (count, self.n_challenges, 4):
                raise ValueError(f"challenges of shape {chal.shape} for {count} witnesses of {self.n_challenges} challenges")
        recs = (Failure * max(1, count * cap))()
        totals = (c_uint32 * (4 * count))()
        fn = lib.zg_prover_check_circuit_dev if device else lib.zg_prover_check_circuit
        _check(fn(self.h, c_size_t(count), adv_ptrs, inst_ptrs, c_size_t(inst_len), _ptr(chal) if chal is not None and chal.size else None,
                  recs if cap else None, c_size_t(cap), totals))
        return self._reports(count, cap, recs, totals, 4)

    def check_phased(self, synthesize, instances, challenges, cap: int = 64):
        """check_circuit with the witness made as prove_phased's is: synthesize(phase, challenges) is called once per phase
        with the caller's challenges uint64[count, n_challenges, 4] and returns, per witness, {advice column: uint64[rows, 4]}
        of the columns of that phase; their usable rows are copied into the slots, which are then checked as they stand
        (the other rows keep what the slots held: they take no part in a shuffle, and a rotation may read them)."""
        count = len(instances)
        n, hip = self.n, _hip_runtime()
        usable = n - (self.image.c.blinding_factors + 1)
        ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(count, self.n_challenges, 4)
        for phase in range(self.phases[0]):
            cols = synthesize(phase, ch.copy())
            for b in range(count):
                for col, values in cols[b].items():
                    if not 0 <= int(col) < self.n_advice:
                        raise ValueError(f"advice column {col} of {self.n_advice}")
                    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)[:usable]
                    if v.shape[0] != usable:
                        raise ValueError(f"advice column {col}: {v.shape[0]} rows, {usable} usable")
                    if hip.hipMemcpy(c_void_p(self.advice_slot(b) + int(col) * n * 32), c_void_p(v.ctypes.data), c_size_t(v.nbytes), 1) != 0:
                        raise ZgError(-2, "hipMemcpy into the advice slot failed")
        return self.check_circuit(None, instances, ch if ch.size else None, cap)

    def check_images(self, plan: "WitnessPlan", images: np.ndarray, cap: int = 64):
        """Wnn::mock_proof for a batch: image bytes -> (reports as check_batch, outputs uint64[count, n_instance, 4])."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        count = images.shape[0]
        images = images.reshape(count, -1)
        outputs = np.zeros((count, plan.n_instance, 4), np.uint64)
        recs = (Failure * max(1, count * cap))()
        totals = (c_uint32 * (3 * count))()
        _check(self.ctx.lib.zg_prover_check_images(self.h, plan.h, _ptr(images), c_size_t(count), _ptr(outputs),
                                                   recs if cap else None, c_size_t(cap), totals))
        return self._reports(count, cap, recs, totals), outputs

    def evaluate_h(self, advice_polys, instance_polys, perm_z_polys, lookup_z_polys, permuted_polys, theta, beta, gamma, y,
                   extended_n: int) -> np.ndarray:
        """Evaluator::evaluate_h / (X^n - 1) from coefficient forms (uint64[count, n, 4] each) -> uint64[extended_n, 4]."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (advice_polys, instance_polys, perm_z_polys, lookup_z_polys,
                                                                    permuted_polys)]
        ptrs = [_ptr(a) if a.size else None for a in arrs]
        out = np.zeros((extended_n, 4), np.uint64)
        _check(self.ctx.lib.zg_prover_evaluate_h(self.h, *ptrs, _ptr(_fr(theta)), _ptr(_fr(beta)), _ptr(_fr(gamma)),
                                                 _ptr(_fr(y)), _ptr(out)))
        return out

    def evaluate_h_dev(self, d_advice_polys: int, d_instance_polys: int, d_perm_z_polys: int, d_lookup_z_polys: int,
                       d_permuted_polys: int, theta, beta, gamma, y, d_h_out: int):
        """evaluate_h with every family and h in HBM (0 = a family the circuit does not have); asynchronous."""
        ptrs = [c_void_p(a) if a else None for a in (d_advice_polys, d_instance_polys, d_perm_z_polys, d_lookup_z_polys,
                                                     d_permuted_polys)]
        _check(self.ctx.lib.zg_prover_evaluate_h_dev(self.h, *ptrs, _ptr(_fr(theta)), _ptr(_fr(beta)), _ptr(_fr(gamma)),
                                                     _ptr(_fr(y)), c_void_p(d_h_out)))

    def lookup_compress_dev(self, lookup: int, d_advice: int, d_instance: int, theta, d_input: int, d_table: int):
        """compress_expressions of lookup `lookup` over the caller's Lagrange columns ([count][2^k] in HBM)."""
        _check(self.ctx.lib.zg_prover_lookup_compress_dev(self.h, c_uint32(lookup), c_void_p(d_advice) if d_advice else None,
                                                          c_void_p(d_instance) if d_instance else None, _ptr(_fr(theta)),
                                                          c_void_p(d_input), c_void_p(d_table)))

    def permutation_sets(self) -> int:
        return int(self.ctx.lib.zg_prover_permutation_sets(self.h))

    def permutation_terms_dev(self, s: int, d_advice: int, d_instance: int, beta, gamma, d_num: int, d_den: int):
        """permutation::prover::commit's factors of column set `s`; chaining the sets is the caller's job."""
        _check(self.ctx.lib.zg_prover_permutation_terms_dev(self.h, c_uint32(s), c_void_p(d_advice) if d_advice else None,
                                                            c_void_p(d_instance) if d_instance else None, _ptr(_fr(beta)),
                                                            _ptr(_fr(gamma)), c_void_p(d_num), c_void_p(d_den)))

    def set_overlap(self, enable, digit_tables: bool = False):
        """True (default): transforms on a side stream (latency); False: one stream per proof (throughput).
        enable == "tables" or digit_tables=True: the latency form AND its digit tables (enable_digit_tables) -- the
        tables are never built implicitly."""
        if enable == "tables":
            enable, digit_tables = True, True
        _check(self.ctx.lib.zg_prover_set_overlap(self.h, ctypes.c_int(1 if enable else 0)))
        if enable and digit_tables:
            self.enable_digit_tables()

    def enable_digit_tables(self, max_bytes: int = 0) -> int:
        """zg_prover_enable_digit_tables: the lone-proof tables of the prover's three base sets (78 GB at k = 14), built NOW;
        max_bytes 0 = the library's cap.  Returns the bytes resident afterwards (0: none fit / none at this size)."""
        built = ctypes.c_uint64(0)
        _check(self.ctx.lib.zg_prover_enable_digit_tables(self.h, ctypes.c_uint64(max_bytes), ctypes.byref(built)))
        return built.value

    def phase_ms(self) -> list:
        out = (ctypes.c_double * 8)()
        _check(self.ctx.lib.zg_prover_phase_ms(self.h, out, c_size_t(8)))
        return list(out)

    def gate_stats(self) -> dict:
        """zg_prover_gate_stats: what the gate (ZG_LAT_GATE) did on this prover so far"""
        out = (ctypes.c_uint64 * 4)()
        _check(self.ctx.lib.zg_prover_gate_stats(self.h, out, c_size_t(4)))
        return dict(zip(("gated_proofs", "gates_armed", "remade_plain", "yields"), (int(x) for x in out)))

    def set_quotient_terms(self, enable: bool):
        """zg_prover_set_quotient_terms: False = every term of the quotient on both parts of the split domain"""
        _check(self.ctx.lib.zg_prover_set_quotient_terms(self.h, ctypes.c_int(1 if enable else 0)))

    def quotient_terms(self) -> dict:
        """zg_prover_quotient_terms: the quotient's terms by degree -- active, and 0 / 1 lists: gates (high), sets and
        lookups (product term high), part2 (per coset slab of a proof: advice, instance, permutation z, lookup z, then
        a'_l, s'_l interleaved -- transformed onto the split domain's second part)"""
        count = c_size_t(0)
        _check(self.ctx.lib.zg_prover_quotient_terms(self.h, None, c_size_t(0), ctypes.byref(count)))
        out = (ctypes.c_uint32 * count.value)()
        _check(self.ctx.lib.zg_prover_quotient_terms(self.h, out, c_size_t(count.value), ctypes.byref(count)))
        v = [int(x) for x in out]
        res, at = {"active": bool(v[0])}, 5
        for name, ln in zip(("gates", "sets", "lookups", "part2"), v[1:5]):
            res[name] = v[at:at + ln]
            at += ln
        return res

    def vk_commitments(self):
        """keygen_vk's commitments: (fixed uint64[n_fixed, 8], sigma uint64[n_perm_columns, 8]), affine."""
        c = self.image.c
        fixed = np.zeros((c.n_fixed, 8), np.uint64)
        sigma = np.zeros((c.n_perm_columns, 8), np.uint64)
        _check(self.ctx.lib.zg_prover_vk_commitments(self.h, _ptr(fixed), _ptr(sigma)))
        return fixed, sigma

    def coset_generator(self) -> np.ndarray:
        """zg_prover_coset_generator: g_coset of the proving key (the creating context's, when the key was made)."""
        out = np.zeros(4, np.uint64)
        _check(self.ctx.lib.zg_prover_coset_generator(self.h, _ptr(out)))
        return out

    def export_key(self, family: int, index: int = 0) -> np.ndarray:
        """zg_prover_export_key: one array of what keygen_pk derived -- KEY_FIXED_POLY / KEY_SIGMA_POLY: uint64[2^k, 4]
        coefficients; KEY_FIXED_COSET / KEY_SIGMA_COSET / KEY_L0 / KEY_L_LAST / KEY_L_ACTIVE_ROW: uint64[2^ext_k, 4] on
        coset_generator() * <extended_omega>."""
        c = self.image.c
        count = self.n
        if family not in (KEY_FIXED_POLY, KEY_SIGMA_POLY):
            while count < self.n * (c.cs_degree - 1):
                count *= 2
        out = np.zeros((count, 4), np.uint64)
        _check(self.ctx.lib.zg_prover_export_key(self.h, c_uint32(family), c_uint32(index), _ptr(out), c_size_t(count)))
        return out

    def fetch(self, what: int, index: int, count: int, slot: int = 0) -> np.ndarray:
        out = np.zeros((count, 4), np.uint64)
        _check(self.ctx.lib.zg_prover_fetch_slot(self.h, c_size_t(slot), c_uint32(what), c_uint32(index), _ptr(out),
                                                 c_size_t(count)))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.zg_prover_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Verifier:
    """zg_verifier: batched GWC verification of proofs of one circuit (circuit.py CircuitImage) on one GPU."""

    def __init__(self, ctx: Ctx, image, fixed_c: np.ndarray, sigma_c: np.ndarray, g0: np.ndarray, g2: np.ndarray,
                 s_g2: np.ndarray, vk_repr: np.ndarray, shuffles=None):
        """fixed_c / sigma_c: uint64[.., 8] affine commitments (Prover.vk_commitments); g0: uint64[8] = g[0];
        g2, s_g2: uint64[16] G2 affine points of the parameters; shuffles: as Prover's (zg_verifier_create_shuffles)."""
        self.ctx = ctx
        self.image = image
        lib = ctx.lib
        lib.zg_verifier_destroy.argtypes = [c_void_p]
        lib.zg_verifier_destroy.restype = None
        arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (fixed_c, sigma_c, g0, g2, s_g2)]
        h = c_void_p()
        if shuffles is not None:
            sh = shuffles if isinstance(shuffles, tuple) else shuffle_array(shuffles)
            _check(lib.zg_verifier_create_shuffles(ctx.h, image.ptr(), sh[0], c_uint32(sh[1]), *[_ptr(a) for a in arrs],
                                                   _ptr(_fr(vk_repr)), ctypes.byref(h)))
        else:
            _check(lib.zg_verifier_create(ctx.h, image.ptr(), *[_ptr(a) for a in arrs], _ptr(_fr(vk_repr)),
                                          ctypes.byref(h)))
        self.h = h
        ctx._adopt(self)

    def set_multiopen(self, scheme: int):
        """zg_verifier_set_multiopen: which multi-open argument the proofs end with (MULTIOPEN_GWC / MULTIOPEN_SHPLONK)."""
        self.ctx.lib.zg_verifier_set_multiopen.argtypes = [c_void_p, ctypes.c_int]
        _check(self.ctx.lib.zg_verifier_set_multiopen(self.h, ctypes.c_int(scheme)))

    @property
    def multiopen(self) -> int:
        self.ctx.lib.zg_verifier_multiopen.argtypes = [c_void_p]
        return int(self.ctx.lib.zg_verifier_multiopen(self.h))

    def set_transcript(self, transcript: int):
        """zg_verifier_set_transcript: which transcript the proofs were written into (TRANSCRIPT_EVM / TRANSCRIPT_BLAKE2B)."""
        self.ctx.lib.zg_verifier_set_transcript.argtypes = [c_void_p, ctypes.c_int]
        _check(self.ctx.lib.zg_verifier_set_transcript(self.h, ctypes.c_int(transcript)))

    @property
    def transcript(self) -> int:
        self.ctx.lib.zg_verifier_transcript.argtypes = [c_void_p]
        return int(self.ctx.lib.zg_verifier_transcript(self.h))

    def set_phases(self, advice_phase, challenge_phase):
        """zg_verifier_set_phases: the phases the proofs were made in (Prover.set_phases' arguments)."""
        _set_phases(self.ctx.lib.zg_verifier_set_phases, self.h, self.image.c.n_advice, advice_phase, challenge_phase)

    @property
    def phases(self):
        return _phases(self.ctx.lib.zg_verifier_phases, self.h, self.image.c.n_advice)

    def verify(self, proofs, instances, key) -> list:
        """Verdict per proof: 1 accepted, 0 rejected, < 0 malformed.  instances[b]: uint64[n_instance, len, 4];
        key: 32 bytes from a CSPRNG (an int in tests, as rng_key)."""
        count = len(proofs)
        bufs = [bytes(p) for p in proofs]
        pptrs = (ctypes.c_char_p * count)(*bufs)
        lens = (c_size_t * count)(*[len(p) for p in bufs])
        insts, inst_len = [], 0
        for b in range(count):
            i, inst_len = Prover._inst(instances[b])
            insts.append(i)
        iptrs = (c_void_p * count)(*[c_void_p(i.ctypes.data) for i in insts])
        verdicts = (c_int * count)()
        _check(self.ctx.lib.zg_verifier_verify_batch(self.h, c_size_t(count), pptrs, lens, iptrs, c_size_t(inst_len),
                                                     rng_key(key), verdicts))
        return list(verdicts)

    def verify_multi(self, proofs, instances, key, circuits: int) -> list:
        """verify for proofs of `circuits` instances each (Prover.prove_multi): instances[b] = the list of proof b's
        per-circuit instance arrays.  Verdicts as verify."""
        return self._verify_several(self.ctx.lib.zg_verifier_verify_multi, proofs, instances, key, circuits)

    def verify_circuits(self, proofs, instances, key, circuits: int) -> list:
        """zg_verifier_verify_circuits: verify_multi for the proofs of Prover.prove_circuits* -- circuits with shuffles,
        challenges and advice phases included."""
        return self._verify_several(self.ctx.lib.zg_verifier_verify_circuits, proofs, instances, key, circuits)

    def _verify_several(self, fn, proofs, instances, key, circuits: int) -> list:
        count = len(proofs)
        bufs = [bytes(p) for p in proofs]
        pptrs = (ctypes.c_char_p * count)(*bufs)
        lens = (c_size_t * count)(*[len(p) for p in bufs])
        insts, inst_len = [], 0
        for b in range(count):
            assert len(instances[b]) == circuits, "one instance array per circuit of every proof"
            for c in range(circuits):
                i, inst_len = Prover._inst(instances[b][c])
                insts.append(i)
        iptrs = (c_void_p * max(len(insts), 1))(*[c_void_p(i.ctypes.data) for i in insts])
        verdicts = (c_int * count)()
        _check(fn(self.h, c_size_t(count), c_size_t(circuits), pptrs, lens, iptrs, c_size_t(inst_len), rng_key(key), verdicts))
        return list(verdicts)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.zg_verifier_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class Wnn:
    """zg_wnn: the cleartext model (Wnn::predict and the compute-accuracy loop) on one GPU.  `model` is an object with the
    fields of harness/wnn_model.Wnn (num_classes, num_filter_entries, num_filter_hashes, num_filter_inputs, p, bloom_filters
    (classes, filters, entries), input_permutation, binarization_thresholds (w, h, bits_per_input)), or a dict of those."""

    FIELDS = ("num_classes", "num_filter_entries", "num_filter_hashes", "num_filter_inputs", "p", "bloom_filters",
              "input_permutation", "binarization_thresholds")

    def __init__(self, ctx: Ctx, model=None, **arrays):
        self.ctx = ctx
        lib = ctx.lib
        lib.zg_wnn_destroy.argtypes = [c_void_p]
        lib.zg_wnn_destroy.restype = None
        get = (lambda f: model[f]) if isinstance(model, dict) else (lambda f: getattr(model, f))
        v = {f: arrays[f] if f in arrays else get(f) for f in self.FIELDS}
        bloom = np.ascontiguousarray(v["bloom_filters"], dtype=np.uint8)
        perm = np.ascontiguousarray(v["input_permutation"], dtype=np.uint64)
        thr = np.ascontiguousarray(v["binarization_thresholds"], dtype=np.uint16)
        assert thr.ndim == 3 and bloom.ndim == 3 and perm.ndim == 1, "thresholds (w, h, bpi), bloom (classes, filters, entries)"
        self.num_classes = int(v["num_classes"])
        self.width, self.height, self.bits_per_input = (int(x) for x in thr.shape)
        n, entries = int(v["num_filter_inputs"]), int(v["num_filter_entries"])
        bits = self.width * self.height * self.bits_per_input
        # the C entry takes pointers: the arrays must have the sizes it will read
        assert perm.shape[0] == bits, "input_permutation has one entry per thermometer bit"
        assert n < 1 or bloom.shape == (self.num_classes, bits // n, entries), "bloom_filters is (classes, filters, entries)"
        h = c_void_p()
        _check(lib.zg_wnn_create(ctx.h, c_uint32(self.num_classes), c_uint32(self.width), c_uint32(self.height),
                                 c_uint32(self.bits_per_input), c_uint32(n), c_uint32(entries),
                                 c_uint32(int(v["num_filter_hashes"])), ctypes.c_uint64(int(v["p"])), _ptr(bloom), _ptr(perm),
                                 _ptr(thr), ctypes.byref(h)))
        self.h = h
        ctx._adopt(self)

    def _images(self, images) -> np.ndarray:
        images = np.ascontiguousarray(images, dtype=np.uint8)
        images = images.reshape(-1, self.width * self.height) if images.size else images.reshape(0, self.width * self.height)
        return images

    def predict(self, images) -> np.ndarray:
        """images: uint8[count, w, h] (or [count, w*h]); returns the class scores, uint64[count, num_classes]."""
        images = self._images(images)
        scores = np.zeros((images.shape[0], self.num_classes), np.uint64)
        _check(self.ctx.lib.zg_wnn_predict(self.h, _ptr(images), c_size_t(images.shape[0]), _ptr(scores)))
        return scores

    def predict_dev(self, d_images: int, count: int, d_scores: int):
        """Device addresses (count * w * h bytes in, count * num_classes uint64 out); asynchronous: Ctx.sync() before reading."""
        _check(self.ctx.lib.zg_wnn_predict_dev(self.h, c_void_p(d_images), c_size_t(count), c_void_p(d_scores)))

    def accuracy(self, images, labels, predictions: bool = True, confusion: bool = True):
        """(correct, predictions uint32[count] or None, confusion uint64[classes, classes] (label, prediction) or None)."""
        images = self._images(images)
        labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        assert labels.shape[0] == images.shape[0], "one label per image"
        pred = np.zeros(images.shape[0], np.uint32) if predictions else None
        conf = np.zeros((self.num_classes, self.num_classes), np.uint64) if confusion else None
        correct = ctypes.c_uint64(0)
        _check(self.ctx.lib.zg_wnn_accuracy(self.h, _ptr(images), _ptr(labels), c_size_t(images.shape[0]),
                                            _ptr(pred) if predictions else None, ctypes.byref(correct),
                                            _ptr(conf) if confusion else None))
        return int(correct.value), pred, conf

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.zg_wnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class Bases:
    def __init__(self, ctx: Ctx, h: c_void_p):
        self.ctx = ctx
        self.h = h

    def __len__(self):
        return self.ctx.lib.zg_bases_len(self.h)

    @property
    def window_bits(self) -> int:
        return self.ctx.lib.zg_bases_window_bits(self.h)

    def free(self):
        if self.h:
            self.ctx.lib.zg_bases_free(self.h)
            self.h = None
