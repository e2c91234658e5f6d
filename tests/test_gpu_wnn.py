"""The cleartext model on the device (zg_wnn_create / zg_wnn_predict / zg_wnn_predict_dev / zg_wnn_accuracy): batched
Wnn::predict and the compute-accuracy loop.  The judge is harness/wnn_model.Wnn.predict, the mirror of wnn.rs that
tests/test_wnn_model.py pins to the reference's own snapshot_mnist_*_predictions; the arithmetic is integer, so every
comparison is exact."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # (before the first HIP call of the process)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKED_IN = {"tiny": "MNIST_TINY", "small": "MNIST_SMALL", "medium": "MNIST_MEDIUM"}


def _model(name):
    import wnn_model

    if name == "synthetic":  # 49-bit filter inputs, p = 2^53 - 111, 4 hashes, 96 filters: more than a wave
        return wnn_model.synthetic_wnn()
    return wnn_model.load_checked_in(getattr(wnn_model, CHECKED_IN[name])[1])


def _mirror(wnn, images) -> np.ndarray:
    return np.array([wnn.predict(im) for im in images], dtype=np.uint64).reshape(len(images), wnn.num_classes)


def _argmax(scores: np.ndarray) -> np.ndarray:
    """utils.rs:35-45: the first index of the strict maximum, 0 when every score is 0 (numpy's argmax is that rule)"""
    return np.argmax(scores, axis=1).astype(np.uint32)


def _predict_dev(ctx, dev, images: np.ndarray, rows: int = None, sentinel: int = -1) -> np.ndarray:
    """Through torch tensors; `rows` >= count rows of output, pre-filled with the sentinel."""
    count = images.shape[0]
    rows = count if rows is None else rows
    d_img = torch.from_numpy(np.ascontiguousarray(images).reshape(-1).copy()).cuda() if count else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_sc = torch.full((max(rows, 1) * dev.num_classes,), sentinel, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dev.predict_dev(d_img.data_ptr(), count, d_sc.data_ptr())
    ctx.sync()
    return d_sc.cpu().numpy().view(np.uint64)[: rows * dev.num_classes].reshape(rows, dev.num_classes)


# ---- 1. the reference's own snapshots
@pytest.mark.parametrize("name", ["tiny", "small", "medium"])
def test_reference_snapshots(ctx, zg, name):
    import wnn_model

    with open(os.path.join(HERE, "golden", "vectors.json")) as f:
        want = json.load(f)["reference"]["predictions"][getattr(wnn_model, CHECKED_IN[name])[1]]
    dev = zg.Wnn(ctx, _model(name))
    got = dev.predict(wnn_model.load_test_image()[None])
    assert got.dtype == np.uint64 and got.tolist() == [want]
    correct, pred, _ = dev.accuracy(wnn_model.load_test_image()[None], [7])
    assert pred.tolist() == [7] and correct == 1  # the image is a seven
    dev.close()


# ---- 2. real shapes
@pytest.mark.parametrize("name", ["tiny", "small", "medium", "synthetic"])
def test_real_shapes_host_and_device_forms(ctx, zg, name):
    import wnn_model

    wnn = _model(name)
    real = wnn_model.load_test_image()
    rng = np.random.default_rng(5)
    images = np.stack([real, np.zeros_like(real), np.full_like(real, 255)] +
                      [rng.integers(0, 256, size=real.shape, dtype=np.uint8) for _ in range(5)])
    want = _mirror(wnn, images)
    dev = zg.Wnn(ctx, wnn)
    assert np.array_equal(dev.predict(images), want)
    assert np.array_equal(_predict_dev(ctx, dev, images), want)
    dev.close()


# ---- 3. the smallest shapes at which the kernel can go wrong
#        (classes, W, H, bpi, n, entries, hashes, p, bloom density)
SMALL_CASES = {
    "64-bit-index-and-prime": (3, 8, 8, 2, 64, 100, 3, 2**64 - 59, 0.7),   # a wrong 128-bit product shows here
    "entries^hashes-over-2^64": (2, 6, 6, 2, 12, 65536, 5, 2**61 - 1, 0.9),  # 2^80: the last index is 0
    "non-square-trailing-bits": (5, 4, 7, 1, 5, 16, 2, 251, 0.7),           # 28 bits, 5 filters, 3 bits dropped
    "one-class": (1, 4, 4, 1, 4, 8, 1, 13, 0.6),
    "33-classes": (33, 6, 6, 2, 3, 8, 1, 7, 0.6),                           # just past a 32-bit class word
    "64-classes-200-filters": (64, 20, 20, 1, 2, 4, 2, 5, 0.7),             # four lane-loop trips, a ragged last one
    "65-filters": (4, 13, 10, 1, 2, 4, 1, 3, 0.6),
}


def _small_model(case, model_seed=7, bloom=None):
    import wnn_model

    classes, w, h, bpi, n, entries, hashes, p, density = SMALL_CASES[case]
    rng = np.random.default_rng(model_seed)
    bits = w * h * bpi
    filters = bits // n
    if bloom is None:
        bloom = rng.random((classes, filters, entries)) < density
    if case == "non-square-trailing-bits":
        thr = rng.choice(np.array([0, 1, 255, 256], dtype=np.uint16), size=(w, h, bpi))
    else:
        thr = rng.integers(0, 257, (w, h, bpi)).astype(np.uint16)
    order = rng.integers(0, bits, bits).astype(np.uint64)  # any in-range map, not a permutation
    return wnn_model.Wnn(classes, entries, hashes, n, p, bloom, order, thr)


def _small_images(case, image_seed=11):
    _, w, h = SMALL_CASES[case][:3]
    rng = np.random.default_rng(image_seed)
    noise = [rng.integers(0, 256, size=(w, h), dtype=np.uint8) for _ in range(6)]
    return np.stack(noise + [np.zeros((w, h), np.uint8), np.full((w, h), 255, np.uint8)])


def _assert_mirror_discriminates(wnn, want):
    """A case whose expected rows are all alike proves nothing: asserted on the mirror, before the device is looked at."""
    filters = wnn.bloom_filters.shape[1]
    assert len({tuple(r) for r in want.tolist()}) >= 3, "fewer than 3 distinct score rows"
    assert not (want == 0).all() and not (want == filters).all()


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_small_shapes(ctx, zg, case):
    wnn = _small_model(case)
    images = _small_images(case)
    want = _mirror(wnn, images)
    _assert_mirror_discriminates(wnn, want)
    dev = zg.Wnn(ctx, wnn)
    got = dev.predict(images)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(_predict_dev(ctx, dev, images), want)
    dev.close()


# ---- 4. batch boundaries
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_batch_boundaries(ctx, zg, count):
    case = "65-filters"
    wnn = _small_model(case)
    base = _small_images(case)
    want8 = _mirror(wnn, base)
    _assert_mirror_discriminates(wnn, want8)
    images = base[np.arange(count) % 8] if count else np.zeros((0,) + base.shape[1:], np.uint8)
    want = want8[np.arange(count) % 8]
    dev = zg.Wnn(ctx, wnn)
    sentinel = 0x5A5A5A5A5A5A5A5A
    rows = count + 3
    # host form, straight through the C entry into an oversized buffer
    buf = np.full((rows, wnn.num_classes), sentinel, np.uint64)
    flat = np.ascontiguousarray(images).reshape(count, base.shape[1] * base.shape[2])
    st = ctx.lib.zg_wnn_predict(dev.h, ctypes.c_void_p(flat.ctypes.data), ctypes.c_size_t(count), ctypes.c_void_p(buf.ctypes.data))
    assert st == 0
    assert np.array_equal(buf[:count], want) and (buf[count:] == sentinel).all()
    # device form
    got = _predict_dev(ctx, dev, flat, rows=rows, sentinel=sentinel)
    assert np.array_equal(got[:count], want) and (got[count:] == sentinel).all()
    assert dev.predict(images).shape == (count, wnn.num_classes)
    dev.close()


# ---- 5. accuracy
@pytest.mark.parametrize("bloom", ["seeded", "all-ones", "all-zeros"])
def test_accuracy(ctx, zg, bloom):
    case = "non-square-trailing-bits"
    classes, w, h, bpi, n, entries = SMALL_CASES[case][:6]
    filters = w * h * bpi // n
    fill = {"seeded": None, "all-ones": np.ones((classes, filters, entries), bool), "all-zeros": np.zeros((classes, filters, entries), bool)}[bloom]
    wnn = _small_model(case, bloom=fill)
    base = _small_images(case)
    want8 = _mirror(wnn, base)
    if bloom == "seeded":
        _assert_mirror_discriminates(wnn, want8)
    elif bloom == "all-ones":
        assert (want8 == filters).all()  # every class ties at `filters`: the prediction is 0
    else:
        assert (want8 == 0).all()        # every score is 0: the prediction is 0
    count = 300
    idx = np.arange(count) % 8
    images = base[idx]
    labels = np.random.default_rng(23).integers(0, classes, count).astype(np.uint32)
    labels[:8] = _argmax(want8)  # (some hits whatever the seed)
    want_pred = _argmax(want8)[idx]
    want_conf = np.zeros((classes, classes), np.uint64)
    np.add.at(want_conf, (labels, want_pred), 1)
    want_correct = int((want_pred == labels).sum())
    if bloom != "seeded":
        assert (want_pred == 0).all()
    dev = zg.Wnn(ctx, wnn)
    correct, pred, conf = dev.accuracy(images, labels)
    assert correct == want_correct and np.array_equal(pred, want_pred) and np.array_equal(conf, want_conf)
    correct, pred, conf = dev.accuracy(images, labels, predictions=False)   # predictions = NULL
    assert correct == want_correct and pred is None and np.array_equal(conf, want_conf)
    correct, pred, conf = dev.accuracy(images, labels, confusion=False)     # confusion = NULL
    assert correct == want_correct and np.array_equal(pred, want_pred) and conf is None
    assert dev.accuracy(images[:0], labels[:0])[0] == 0
    dev.close()


# ---- 6. validation
def _create_raw(context, **over):
    """zg_wnn_create through ctypes with one argument replaced; returns (status, handle)."""
    lib = context.lib
    a = dict(ctx=context.h, num_classes=3, width=4, height=4, bits_per_input=2, num_filter_inputs=4, num_filter_entries=8,
             num_filter_hashes=2, p=13)
    a.update({k: v for k, v in over.items() if k in a})
    bits = a["width"] * a["height"] * a["bits_per_input"]
    n = a["num_filter_inputs"]
    filters = bits // n if n else 1
    keep = dict(bloom=np.ones((max(a["num_classes"], 1), max(filters, 1), max(a["num_filter_entries"], 1)), np.uint8),
                perm=np.arange(max(bits, 1), dtype=np.uint64), thr=np.full(max(bits, 1), 100, np.uint16))
    keep.update({k: v for k, v in over.items() if k in keep})
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)
    h = ctypes.c_void_p()
    st = lib.zg_wnn_create(a["ctx"], ctypes.c_uint32(a["num_classes"]), ctypes.c_uint32(a["width"]), ctypes.c_uint32(a["height"]),
                               ctypes.c_uint32(a["bits_per_input"]), ctypes.c_uint32(n), ctypes.c_uint32(a["num_filter_entries"]),
                               ctypes.c_uint32(a["num_filter_hashes"]), ctypes.c_uint64(a["p"]), ptr(keep["bloom"]), ptr(keep["perm"]),
                               ptr(keep["thr"]), None if over.get("out") == "null" else ctypes.byref(h))
    return st, h


def test_validation(ctx, zg):
    INVALID, UNSUPPORTED = -1, -4
    lib = ctx.lib
    lib.zg_wnn_destroy.argtypes = [ctypes.c_void_p]
    lib.zg_wnn_destroy.restype = None
    st, h = _create_raw(ctx)
    assert st == 0 and h.value
    lib.zg_wnn_destroy(h)
    bad_perm = np.arange(32, dtype=np.uint64)
    bad_perm[17] = 32
    bad_thr = np.full(32, 100, np.uint16)
    bad_thr[31] = 257
    refusals = [
        (dict(ctx=None), INVALID), (dict(bloom=None), INVALID), (dict(perm=None), INVALID), (dict(thr=None), INVALID),
        (dict(out="null"), INVALID),
        (dict(num_classes=0), INVALID), (dict(width=0), INVALID), (dict(height=0), INVALID), (dict(bits_per_input=0), INVALID),
        (dict(num_filter_entries=0), INVALID), (dict(num_filter_hashes=0), INVALID), (dict(p=0), INVALID),
        (dict(num_filter_inputs=0), INVALID), (dict(num_filter_inputs=65), INVALID),
        (dict(width=1, height=1, bits_per_input=1, num_filter_inputs=2), INVALID),  # one bit makes no filter of two inputs
        (dict(perm=bad_perm), INVALID), (dict(thr=bad_thr), INVALID),
        (dict(num_classes=65), UNSUPPORTED),
    ]
    seen = set()
    for over, want in refusals:
        st, h = _create_raw(ctx, **over)
        assert st == want, (over.keys(), st)
        assert not h.value
        # (this refusal's own message, not one left over from the refusal before: each names what it refused)
        msg = lib.zg_last_error().decode()
        assert msg.startswith("zg_wnn_create: ") and msg not in seen, (over.keys(), msg)
        seen.add(msg)
    # ... and on a model: a label outside the classes, null arrays
    wnn = _small_model("65-filters")
    images = _small_images("65-filters")
    dev = zg.Wnn(ctx, wnn)
    with pytest.raises(zg.ZgError) as e:
        dev.accuracy(images, [0, 1, 2, 3, 4, 0, 0, 0])  # 4 classes: label 4 is out of range
    assert e.value.status == INVALID and "label" in str(e.value)
    flat = images.reshape(8, -1)
    scores = np.zeros((8, 4), np.uint64)
    assert lib.zg_wnn_predict(dev.h, None, ctypes.c_size_t(8), ctypes.c_void_p(scores.ctypes.data)) == INVALID and lib.zg_last_error()
    assert lib.zg_wnn_predict(dev.h, ctypes.c_void_p(flat.ctypes.data), ctypes.c_size_t(8), None) == INVALID
    assert lib.zg_wnn_predict(None, ctypes.c_void_p(flat.ctypes.data), ctypes.c_size_t(8), ctypes.c_void_p(scores.ctypes.data)) == INVALID
    assert lib.zg_wnn_predict_dev(dev.h, None, ctypes.c_size_t(8), None) == INVALID and lib.zg_last_error()
    correct = ctypes.c_uint64(0)
    labels = np.zeros(8, np.uint32)
    assert lib.zg_wnn_accuracy(dev.h, ctypes.c_void_p(flat.ctypes.data), ctypes.c_void_p(labels.ctypes.data), ctypes.c_size_t(8), None, None, None) == INVALID
    assert lib.zg_wnn_accuracy(dev.h, None, ctypes.c_void_p(labels.ctypes.data), ctypes.c_size_t(8), None, ctypes.byref(correct), None) == INVALID
    # the same context and the same model still work afterwards
    assert np.array_equal(dev.predict(images), _mirror(wnn, images))
    dev.close()


# ---- 7. what gets proven is what predict says
def test_scores_equal_the_proof_path_instance_values(ctx, zg):
    import witness_tape
    import wnn_model

    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    real = wnn_model.load_test_image()
    rng = np.random.default_rng(3)
    images = np.stack([real] + [rng.integers(0, 256, size=real.shape, dtype=np.uint8) for _ in range(2)])
    plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    n = 1 << k
    bufs = [torch.zeros(plan.n_advice * n * 4, dtype=torch.int64, device="cuda") for _ in images]
    torch.cuda.synchronize()
    inst = plan.run(images, [b.data_ptr() for b in bufs])
    proven = [[zg.fr_to_int(x) for x in row] for row in inst]  # (out of Montgomery form)
    dev = zg.Wnn(ctx, wnn)
    assert dev.predict(images).tolist() == proven
    plan.close()
    dev.close()
