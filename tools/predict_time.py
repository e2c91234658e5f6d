#!/usr/bin/env python3
"""What scoring a test set costs on the device:   python tools/predict_time.py [--out PATH] [--models tiny,small,medium,large]
                                                                               [--images N] [--witness-images M]

Per model, ONE process, a warm-up and three samples each, host clock around blocking calls; a sample is CALLS (20)
calls back to back -- one call is a fraction of a millisecond -- and every figure is per call.  N seeded noise images plus
benches/example_image_7 (10 001 by default):
  predict          zg_wnn_predict: host arrays in and out
  predict_dev      zg_wnn_predict_dev + zg_ctx_sync: device arrays in and out (the kernel and its launch)
  predict_kernel   the wnn_predict kernel alone (its own HIP events, zg_ctx_profile_*), in a pass of its own
  accuracy         zg_wnn_accuracy with predictions and the confusion matrix
  witness_run      the FIRST M of the same images (1024 by default) through WitnessPlan.run, 64 per call into resident
                   advice buffers: the only device route to class scores before the model object existed.  It also writes
                   the advice columns of a proof, which is what it is for; the figure is what a caller who wanted scores paid.
Scores of the device forms are compared with each other, with the witness program's instance values and (first 8 images)
with the host mirror.  `large` is the seeded stand-in of harness/wnn_model.synthetic_wnn.  No speed condition is asserted.
Writes profiles/r12/predict_time.json (or PATH)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("0g-halo2_amd", "harness"):
    sys.path.insert(0, os.path.join(ROOT, d))
import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)

import numpy as np  # noqa: E402
import witness_tape  # noqa: E402
import wnn_model  # noqa: E402
import zg_halo2 as zg  # noqa: E402

REPS = 3
CALLS = 20  # calls per sample
MODELS = {"tiny": wnn_model.MNIST_TINY, "small": wnn_model.MNIST_SMALL, "medium": wnn_model.MNIST_MEDIUM, "large": wnn_model.MNIST_LARGE}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn, reps=REPS):
    fn()  # warm: workspace, code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        out.append((time.perf_counter() - t0) / CALLS)
    return out


def entry(times, images):
    med = statistics.median(times)
    return {"median_ms": round(med * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times], "images": images,
            "images_per_s": round(images / med)}


def one_model(ctx, label, images, witness_images):
    k, name = MODELS[label]
    wnn = wnn_model.synthetic_wnn() if label == "large" else wnn_model.load_checked_in(name)
    count = images.shape[0]
    classes, filters, entries = wnn.bloom_filters.shape
    pixels = images.shape[1] * images.shape[2]
    dev = zg.Wnn(ctx, wnn)
    word = 4 if classes <= 32 else 8
    res = {"model": name, "k": k, "classes": classes, "filters": filters, "entries": entries, "hashes": wnn.num_filter_hashes,
           "filter_inputs": wnn.num_filter_inputs,
           "bloom_table_bytes": filters * entries * word, "encode_table_bytes": filters * wnn.num_filter_inputs * 4,
           # what the algorithm moves per image: the pixels in, the scores out (the tables are resident)
           "bytes_per_image": {"in": pixels, "out": 8 * classes}}
    got = {}

    def host():
        got["host"] = dev.predict(images)

    res["predict"] = entry(timed(host), count)
    d_img = torch.from_numpy(images.reshape(-1).copy()).cuda()
    d_sc = torch.zeros(count * classes, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def device():
        dev.predict_dev(d_img.data_ptr(), count, d_sc.data_ptr())
        ctx.sync()

    res["predict_dev"] = entry(timed(device), count)
    assert np.array_equal(d_sc.cpu().numpy().view(np.uint64).reshape(count, classes), got["host"])
    assert got["host"][:8].tolist() == [wnn.predict(im) for im in images[:8]]
    ctx.profile(True)
    for _ in range(REPS):
        device()
    launches, total_ms = ctx.profile_collect()["wnn_predict"][:2]
    ctx.profile(False)
    res["predict_kernel"] = {"mean_ms": round(total_ms / launches, 4), "launches": launches, "images": count,
                             "images_per_s": round(count / (total_ms / launches * 1e-3))}
    labels = (np.arange(count) % classes).astype(np.uint32)

    def accuracy():
        got["acc"] = dev.accuracy(images, labels)

    res["accuracy"] = entry(timed(accuracy), count)
    assert np.array_equal(got["acc"][1], np.argmax(got["host"], axis=1))
    dev.close()

    # the route that existed before: the recorded witness program, 64 images per call
    m = min(witness_images, count)
    plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    n = 1 << k
    bufs = [torch.zeros(plan.n_advice * n * 4, dtype=torch.int64, device="cuda") for _ in range(min(64, m))]
    ptrs = [b.data_ptr() for b in bufs]
    torch.cuda.synchronize()

    def witness():
        out = []
        for i in range(0, m, 64):
            chunk = images[i:i + 64]
            out.append(plan.run(chunk, ptrs[: chunk.shape[0]]))
        got["witness"] = np.concatenate(out)

    res["witness_run"] = entry(timed(witness), m)
    res["witness_run"]["bytes_per_image"] = {"in": pixels, "out": 32 * classes, "advice_columns_written": plan.n_advice * n * 32}
    proven = np.array([[zg.fr_to_int(x) for x in row] for row in got["witness"]], dtype=np.uint64)
    assert np.array_equal(proven, got["host"][:m]), "the witness program and predict disagree"
    plan.close()
    del bufs
    torch.cuda.empty_cache()
    res["predict_over_witness_run"] = round(res["predict"]["images_per_s"] / res["witness_run"]["images_per_s"], 1)
    return res


def main():
    out = arg("--out", os.path.join(ROOT, "profiles", "r12", "predict_time.json"))
    labels = arg("--models", "tiny,small,medium,large").split(",")
    count, witness_images = int(arg("--images", "10000")), int(arg("--witness-images", "1024"))
    real = wnn_model.load_test_image()
    rng = np.random.default_rng(12)
    images = np.concatenate([real[None], rng.integers(0, 256, size=(count,) + real.shape, dtype=np.uint8)])
    ctx = zg.Ctx(0)
    res = {"reps": REPS, "calls_per_sample": CALLS, "device": torch.cuda.get_device_name(0), "images": int(images.shape[0]), "models": {}}
    for label in labels:
        res["models"][label] = one_model(ctx, label, images, witness_images)
        print(label, json.dumps(res["models"][label]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
