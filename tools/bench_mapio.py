#!/usr/bin/env python3
"""What map datasets cost on the host and on the device (peanut_amd/mapio.py, csrc/mapio.hip).  Sides alternate in one process,
medians with [min, max] over ``--repeats`` windows; every shape is warmed up; host clocks around work that ends in a synchronise.

* ``snapshot``  (-> <out>/snapshot.jsonl) a 960 x 960 x 14 full map per episode, E = 1, 4, 8 episodes:
    ``host``             the route of `mapio.encode_map`: `(full_map.cpu().numpy() * 255).astype(np.uint8)`
                         (collect_maps.py:81-82), E times in a row;
    ``device_readback``  one `peanut_mapseq_encode` over the E maps, then the uint8 results copied down (what `encode_map` of a
                         HIP tensor would do on the device route, for E maps);
    ``device_resident``  the recorder's form: one launch into E slots of device sequences, nothing read back.
  ``earns_default``: the ``device_readback`` median lies below the ``host`` median by more than both spreads -- the condition under
  which `encode_map` would take the device route for HIP tensors (it has not been met on every E).
* ``evaluate``  (-> <out>/evaluate.jsonl) files of [20, 14, 960, 960] sequences, the 720 window, fp32, ten samples per file:
    ``evaluate``         `mapio.evaluate` (uint8 upload, inputs / forward / loss on the device);
    ``host_route``       per sample `mapio.model_input` of the crop made on the host and uploaded as fp32, the same forward, the
                         logits copied down, torch's float64 `binary_cross_entropy_with_logits` on `target_from_sequence`;
    ``forward_alone``    the forward of a file's ten samples on inputs already on the device;
    ``load_alone``       `np.load` of the files (both routes contain it).

* ``train_batch``  (``--train-batch`` -> <out>/train_batch.jsonl) the workload's own shape: 960 x 960 x 14 maps, pad 1200, crop
  960, B = 8, K = 6, samples from two compacted sequences [11, 14, 960, 960] on the device:
    ``train_off`` / ``train_on``  one `peanut_mapseq_train_batch` with the rotation off / on (offsets, flips and angles as drawn);
    ``model_input_batch``         the ABI 21 call at the same B and S: the same fp32 bytes, no gather, no target;
    ``host_sample``               the pipeline restated per sample with NumPy and scipy (pad, crop, flip, `affine_transform`), on a
                                  sequence already in memory; ``load_file`` is `np.load` of a [20, 14, 960, 960] file, timed apart.

    python tools/bench_mapio.py [--out profiles/mapio] [--repeats 5] [--snapshot-only | --evaluate-only | --train-batch]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def synth_map(seed, C=14, W=960, dev=None):
    """A full map as an episode leaves it: obstacle / explored discs of values in [0, 1], a trail, a few semantic blobs."""
    rng = np.random.RandomState(seed)
    m = np.zeros((C, W, W), np.float32)
    yy, xx = np.mgrid[:W, :W]
    for _ in range(6):
        r0, c0, rad = rng.randint(200, W - 200), rng.randint(200, W - 200), rng.randint(40, 160)
        disc = (yy - r0) ** 2 + (xx - c0) ** 2 <= rad ** 2
        m[1][disc] = 1.0
        m[0][disc & (rng.uniform(0, 1, (W, W)) > 0.93)] = 1.0
    for k in range(4, C):
        r0, c0 = rng.randint(100, W - 100, 2)
        m[k, r0:r0 + 12, c0:c0 + 12] = rng.uniform(0, 1, (12, 12))
    m[2, W // 2 - 1:W // 2 + 2, W // 2 - 1:W // 2 + 2] = 1.0
    return torch.from_numpy(m).to(dev) if dev is not None else m


def host_encode(full_map):
    """The host route of `mapio.encode_map` (collect_maps.py:81-82)."""
    return (full_map.detach().cpu().numpy() * 255).astype(np.uint8)


def snapshot(dev, repeats, calls=(48, 1500, 20000)):
    from peanut_amd import mapio
    maps = [synth_map(e, dev=dev) for e in range(8)]
    T = 4
    recs = []
    for E in (1, 4, 8):
        seqs = [torch.zeros((T,) + tuple(maps[0].shape), dtype=torch.uint8, device=dev) for _ in range(E)]
        last = {}

        def host(n):
            for _ in range(n):
                last["host"] = [host_encode(m) for m in maps[:E]]

        def device_readback(n):
            for _ in range(n):
                out, _ = mapio.encode_maps_device(maps[:E])
                last["device_readback"] = [o.cpu().numpy() for o in out]

        def device_resident(n):
            for i in range(n):
                mapio.encode_maps_device(maps[:E], out=[q[i % T] for q in seqs])
        # calls per window, per side: every window runs for a good fraction of a second
        per = [max(c // E, 1) for c in calls]                             # (the work of a call grows with E)
        sides = [("host", host, per[0]), ("device_readback", device_readback, per[1]), ("device_resident", device_resident, per[2])]
        for _, fn, _n in sides:
            fn(2)
        torch.cuda.synchronize()
        t = {name: [] for name, _, _n in sides}
        for _ in range(repeats):
            for name, fn, n in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(n)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / n * 1e3)
        sp = {name: spread(v) for name, v in t.items()}
        same = all(np.array_equal(a, b) for a, b in zip(last["host"], last["device_readback"])) and \
            all(np.array_equal(q[0].cpu().numpy(), a) for q, a in zip(seqs, last["host"]))
        noise = (sp["host"]["max"] - sp["host"]["min"]) + (sp["device_readback"]["max"] - sp["device_readback"]["min"])
        rec = {"section": "snapshot", "E": E, "shape": list(maps[0].shape), "calls_per_window": dict(zip(("host", "device_readback", "device_resident"), per)),
               "ms_per_save_step": sp, "host_over_device_readback": round(sp["host"]["median"] / sp["device_readback"]["median"], 2),
               "host_over_device_resident": round(sp["host"]["median"] / sp["device_resident"]["median"], 1),
               "device_resident_GBps": round(E * maps[0].numel() * 5 / sp["device_resident"]["median"] / 1e6, 1),
               "earns_default": bool(sp["host"]["median"] - sp["device_readback"]["median"] > noise), "bits_equal": bool(same)}
        print(f"snapshot, E = {E}: {rec}", file=sys.stderr, flush=True)
        recs.append(rec)
    return recs


def evaluate(dev, repeats, n_files=2, window=720):
    import torch.nn.functional as F
    from types import SimpleNamespace

    from peanut_amd import mapio
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    model = PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=dev.index), state_dict=make_seeded_state_dict(PredCfg(), 0), precision="fp32")
    ts, K = list(range(10)), 6
    tmp = tempfile.mkdtemp(prefix="bench_mapio_")
    files = []
    for f in range(n_files):
        seq = np.stack([(synth_map(100 * f + min(t, 3)) * 255).astype(np.uint8) for t in range(4)])
        seq = seq[[min(t, 3) for t in range(20)]]                       # 20 snapshots; the map stops changing after the fourth
        files.append(os.path.join(tmp, f"f{f:05d}.npz"))
        np.savez_compressed(files[-1], maps=seq)
    W = seq.shape[2]
    x1 = W // 2 - window // 2
    last = {}

    def device_route():
        last["evaluate"] = mapio.evaluate(model, files, t_indices=ts, window=window)

    def host_route():
        total = np.zeros(K)
        for f in files:
            seq = mapio.load_map_sequence(f)
            x = torch.cat([mapio.model_input(seq[:, :, x1:x1 + window, x1:x1 + window], t, device=dev) for t in ts])
            logits = model.get_prediction_batch(x, apply_sigmoid=False).cpu()
            for b, t in enumerate(ts):
                tgt = mapio.target_from_sequence(seq, t, range(4, 4 + K))[x1:x1 + window, x1:x1 + window].transpose(2, 0, 1)
                y = (torch.from_numpy(np.ascontiguousarray(tgt)).float() / 255.).double()
                total += F.binary_cross_entropy_with_logits(logits[b].double(), y, reduction='none').sum(dim=(1, 2)).numpy()
        per = total / (len(files) * len(ts) * window * window)
        last["host_route"] = {"loss": float(per.mean()), "loss_per_channel": [float(v) for v in per]}

    xdev = mapio.model_input_batch(mapio.to_device(mapio.load_map_sequence(files[0]), dev), ts, window=window)

    def forward_alone():
        for _ in files:
            model.get_prediction_batch(xdev, apply_sigmoid=False)

    def load_alone():
        for f in files:
            mapio.load_map_sequence(f)
    sides = [("evaluate", device_route), ("host_route", host_route), ("forward_alone", forward_alone), ("load_alone", load_alone)]
    for _, fn in sides:
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in sides}
    for _ in range(repeats):
        for name, fn in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    n_maps = len(files) * len(ts)
    rec = {"section": "evaluate", "files": len(files), "samples_per_file": len(ts), "window": window, "precision": "fp32",
           "sequence_shape": list(seq.shape),
           "maps_per_s": {name: spread([n_maps / s for s in t[name]]) for name in ("evaluate", "host_route", "forward_alone")},
           "seconds": {name: spread(v) for name, v in t.items()},
           "loss": {"evaluate": last["evaluate"]["loss"], "host_route": last["host_route"]["loss"]},
           "loss_per_channel_max_abs_diff": float(np.abs(np.array(last["evaluate"]["loss_per_channel"]) -
                                                         np.array(last["host_route"]["loss_per_channel"])).max())}
    med = {name: statistics.median(v) for name, v in t.items()}
    rec["seconds_beside_forward_and_load"] = {name: round(med[name] - med["forward_alone"] - med["load_alone"], 4)
                                              for name in ("evaluate", "host_route")}
    print(f"evaluate: {rec}", file=sys.stderr, flush=True)
    for f in files:
        os.remove(f)
    os.rmdir(tmp)
    return [rec]


def host_sample(maps, t, p, pad, crop, K):
    """The reference's pipeline on one sample, restated with NumPy and scipy: fp32 image, uint8 target."""
    import math

    from scipy.ndimage import affine_transform
    W, H = maps.shape[2:]
    img = maps[t].astype(np.float32) / np.float32(255.)
    gt = maps[-1, 4:4 + K] * (maps[t, 1] == 0)
    out = []
    for a, order in ((img, 1), (gt, 0)):
        a = np.pad(a, [(0, 0), (0, pad[0] - W), (0, pad[1] - H)])[:, p["off_r"]:p["off_r"] + crop[0], p["off_c"]:p["off_c"] + crop[1]]
        a = a[:, :, ::-1] if p["flip"] == 1 else a[:, ::-1] if p["flip"] == 2 else a
        if p["rotate"]:
            c, s = math.cos(math.radians(p["angle"])), math.sin(math.radians(p["angle"]))
            cy, cx = (crop[0] - 1) / 2.0, (crop[1] - 1) / 2.0
            off = [cy - c * cy + s * cx, cx - s * cy - c * cx]
            a = np.stack([affine_transform(np.ascontiguousarray(pl), [[c, -s], [s, c]], offset=off, order=order, mode="grid-constant", cval=0)
                          for pl in a])
        out.append(np.ascontiguousarray(a))
    return out


def train_batch(dev, repeats, B=8, calls=100):
    from peanut_amd import mapio
    pad, crop, K, W = (1200, 1200), (960, 960), 6, 960
    full = [np.stack([(synth_map(100 * f + min(t, 3)) * 255).astype(np.uint8) for t in range(4)])[[min(t, 3) for t in range(20)]] for f in range(2)]
    tmp = tempfile.mkdtemp(prefix="bench_mapio_")
    path = os.path.join(tmp, "f00000.npz")
    np.savez_compressed(path, maps=full[0])
    seqs = [mapio.to_device(mapio.compact_sequence(m), dev) for m in full]
    ts = [b % 10 for b in range(B)]
    rows = mapio.TrainAugment(pad, crop, seed=0).draw(B, (W, W))          # the reference's settings: flip 0.5, rotation always
    rows_off = rows.copy()
    rows_off["rotate"] = 0
    img = torch.empty((B, 14) + crop, dtype=torch.float32, device=dev)
    gt = torch.empty((B, K) + crop, dtype=torch.uint8, device=dev)
    batch_seqs = [seqs[b % 2] for b in range(B)]
    host_maps = mapio.compact_sequence(full[0])

    def train_off(n):
        for _ in range(n):
            mapio.train_batch(batch_seqs, ts, rows_off, pad, crop, K=K, img=img, gt=gt)

    def train_on(n):
        for _ in range(n):
            mapio.train_batch(batch_seqs, ts, rows, pad, crop, K=K, img=img, gt=gt)

    def inputs(n):
        for _ in range(n):
            mapio.model_input_batch(seqs[0], ts, window=W, out=img)

    def host(n):
        for i in range(n):
            host_sample(host_maps, ts[i % B], rows[i % B], pad, crop, K)

    def load(n):
        for _ in range(n):
            mapio.load_map_sequence(path)
    sides = [("train_off", train_off, calls), ("train_on", train_on, calls), ("model_input_batch", inputs, calls), ("host_sample", host, 1),
             ("load_file", load, 1)]
    for name, fn, n in sides:
        fn(min(n, 3))
    torch.cuda.synchronize()
    t = {name: [] for name, _, _n in sides}
    for _ in range(repeats):
        for name, fn, n in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / n * 1e3)
    sp = {name: spread(v) for name, v in t.items()}
    cells = B * crop[0] * crop[1]
    written = {"train_off": cells * (14 * 4 + K), "train_on": cells * (14 * 4 + K), "model_input_batch": cells * 14 * 4}
    rec = {"section": "train_batch", "B": B, "map": [14, W, W], "pad": list(pad), "crop": list(crop), "K": K, "calls_per_window": {n: c for n, _, c in sides},
           "ms": sp, "bytes_written_per_call": written,
           "written_GBps": {n: round(b / sp[n]["median"] / 1e6, 1) for n, b in written.items()},
           "train_on_over_model_input_batch": round(sp["train_on"]["median"] / sp["model_input_batch"]["median"], 2),
           "train_off_over_model_input_batch": round(sp["train_off"]["median"] / sp["model_input_batch"]["median"], 2),
           "host_batch_over_train_on": round(B * sp["host_sample"]["median"] / sp["train_on"]["median"], 1)}
    print(f"train_batch: {rec}", file=sys.stderr, flush=True)
    os.remove(path)
    os.rmdir(tmp)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapio"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--snapshot-only", action="store_true")
    ap.add_argument("--evaluate-only", action="store_true")
    ap.add_argument("--train-batch", action="store_true", help="only the train_batch section")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mapio.py measures on the GPU; none is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(a.out, exist_ok=True)
    for name, fn, skip in (("snapshot", snapshot, a.evaluate_only or a.train_batch), ("evaluate", evaluate, a.snapshot_only or a.train_batch),
                           ("train_batch", train_batch, not a.train_batch)):
        if skip:
            continue
        with open(os.path.join(a.out, name + ".jsonl"), "w") as f:
            for r in fn(dev, a.repeats):
                r["device"] = torch.cuda.get_device_name(dev)
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
