"""Augmented training batches (ABI 25) on the device: ``peanut_mapseq_train_batch`` with rotation off against the reference's own
pipeline (tests/golden/train_batch_golden.npz) bit for bit, with rotation on against the float64 restatement of
tests/train_batch_cases.py (image within 1e-6: at most 11 roundings of 2^-24 on terms <= 1; target bit-equal on every cell, which the
tie condition checked in tests/test_train_batch_cpu.py allows), and the layers above it: ``bce_score_target``, ``MapStore``,
``TrainBatcher``, ``evaluate(augment=...)``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_cases as tc                              # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -2
IMG_TOL = 1e-6
ALL_CASES = {**tc.OFF_CASES, **tc.ON_CASES}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(tc.GOLDEN))


def _rows(params):
    from peanut_amd import mapio
    rows = np.zeros(len(params), mapio.PARAMS_DTYPE)
    for row, p in zip(rows, params):
        row["off_r"], row["off_c"], row["flip"], row["rotate"], row["angle"] = p
    return rows


def _golden_params(golden, name):
    p, d = golden[f"{name}/params"], golden[f"{name}/draws"]
    return [(int(a), int(b), int(f), int(r), float(ang)) for (a, b, f, r), ang in zip(p, d[:, 5])]


def _call(seqs, sources, params, pad, crop, K):
    """One ``train_batch`` over outputs prefilled with 0xFF -> (img, gt) on the host.  A cell that stays unwritten is a NaN in img."""
    from peanut_amd import mapio
    devs = [mapio.to_device(s) for s in seqs]
    B, Cn = len(sources), seqs[0].shape[1]
    img = torch.empty((B, Cn) + tuple(crop), dtype=torch.float32, device="cuda")
    gt = torch.empty((B, K) + tuple(crop), dtype=torch.uint8, device="cuda")
    img.view(torch.uint8).fill_(0xFF)
    gt.fill_(0xFF)
    out = mapio.train_batch([devs[k] for k, _ in sources], [t for _, t in sources], _rows(params), pad, crop, K=K, img=img, gt=gt)
    assert out[0] is img and out[1] is gt
    img, gt = img.cpu().numpy(), gt.cpu().numpy()
    assert not np.isnan(img).any(), "img has unwritten cells"
    return img, gt


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(tc.OFF_CASES))
def test_rotation_off_equals_the_reference_pipeline_bit_for_bit(golden, name):
    case = tc.OFF_CASES[name]
    seqs = [golden[f"{name}/seq{k}"] for k in range(len(case["T"]))]
    img, gt = _call(seqs, tc.sample_sources(case), _golden_params(golden, name), case["pad"], case["crop"], case["K"])
    assert _same_bits(img, golden[f"{name}/img"]), np.abs(img - golden[f"{name}/img"]).max()
    assert _same_bits(gt, golden[f"{name}/gt"])


@pytest.mark.parametrize("name", sorted(tc.ON_CASES))
def test_rotation_on_golden_cases_match_the_restatement_and_the_pipeline(golden, name):
    case = tc.ON_CASES[name]
    seqs = [golden[f"{name}/seq{k}"] for k in range(len(case["T"]))]
    params = _golden_params(golden, name)
    img, gt = _call(seqs, tc.sample_sources(case), params, case["pad"], case["crop"], case["K"])
    for i, ((k, t), p) in enumerate(zip(tc.sample_sources(case), params)):
        r = tc.restate(seqs[k], t, *p, case["pad"], case["crop"], case["K"])
        err = float(np.abs(img[i].astype(np.float64) - r["img"]).max())
        print(f"{name} sample {i} angle {p[4]:9.3f} rotate {p[3]}: max |img - restatement| {err:.3e}")
        assert err <= IMG_TOL, (name, i, err)
        assert np.array_equal(gt[i], r["gt"]) and np.array_equal(gt[i], golden[f"{name}/gt"][i]), (name, i)
        if not p[3]:
            assert _same_bits(img[i], golden[f"{name}/img"][i].astype(np.float32))
    assert np.abs(img - golden[f"{name}/img"]).max() <= IMG_TOL + 1e-12      # (the pipeline is within 1e-12 of the restatement)


@pytest.mark.parametrize("shape", sorted(tc.ANGLE_SHAPES))
def test_stated_angles_match_the_restatement(shape):
    sh = tc.ANGLE_SHAPES[shape]
    maps = tc.make_sequence(sh["T"], sh["C"], sh["map"], 77)
    params = tc.angle_params(tc.ANGLES, sh)
    sources = [(0, i % sh["T"]) for i in range(len(params))]
    img, gt = _call([maps], sources, params, sh["pad"], sh["crop"], sh["K"])
    for i, ((_, t), p) in enumerate(zip(sources, params)):
        r = tc.restate(maps, t, *p, sh["pad"], sh["crop"], sh["K"])
        err = float(np.abs(img[i].astype(np.float64) - r["img"]).max())
        print(f"{shape} angle {p[4]:9.3f}: max |img - restatement| {err:.3e}, target cells that differ {int((gt[i] != r['gt']).sum())}")
        assert err <= IMG_TOL, (shape, p, err)
        assert np.array_equal(gt[i], r["gt"]), (shape, p)
        assert r["gt"].any()
    # 0 degrees IS the rotation-off result
    assert params[0][4] == 0.0
    off = [p[:3] + (0,) + p[4:] for p in params[:1]]
    img0, gt0 = _call([maps], sources[:1], off, sh["pad"], sh["crop"], sh["K"])
    assert _same_bits(img0[0], img[0]) and _same_bits(gt0[0], gt[0])


def _mixed_batch(n):
    """n samples of case rot_even's shape from two sequences of different T, rotation on and off, every flip."""
    case = tc.ON_CASES["rot_even"]
    seqs = [tc.make_sequence(T, case["C"], case["map"], 500 + T) for T in (2, 4)]
    rng = np.random.RandomState(9)
    mr, mc = case["pad"][0] - case["crop"][0], case["pad"][1] - case["crop"][1]
    params = [(int(rng.randint(0, mr + 1)), int(rng.randint(0, mc + 1)), int(rng.randint(0, 3)), int(i % 3 != 0), float(rng.uniform(-180, 180)))
              for i in range(n)]
    sources = [(i % 2, i % (2, 4)[i % 2]) for i in range(n)]
    return case, seqs, sources, params


def test_65_samples_equal_64_plus_1_and_a_result_does_not_depend_on_its_slot():
    case, seqs, sources, params = _mixed_batch(65)
    args = (case["pad"], case["crop"], case["K"])
    img, gt = _call(seqs, sources, params, *args)
    img64, gt64 = _call(seqs, sources[:64], params[:64], *args)
    img1, gt1 = _call(seqs, sources[64:], params[64:], *args)
    assert _same_bits(img, np.concatenate([img64, img1])) and _same_bits(gt, np.concatenate([gt64, gt1]))
    # reversed: every sample in another slot (and another launch: 64 becomes the single one's neighbour)
    rimg, rgt = _call(seqs, sources[::-1], params[::-1], *args)
    assert _same_bits(rimg[::-1].copy(), img) and _same_bits(rgt[::-1].copy(), gt)
    one, _ = _call(seqs, sources[7:8], params[7:8], *args)
    assert _same_bits(one[0], img[7])
    assert gt.any() and len({img[i].tobytes() for i in range(65)}) == 65


def test_gt_may_be_absent():
    from peanut_amd import _lib, mapio
    case = tc.OFF_CASES["tall"]
    seq = mapio.to_device(tc.sequences(case)[0])
    img = torch.zeros((1, case["C"]) + case["crop"], dtype=torch.float32, device="cuda")
    d = tc.train_desc(img=img.data_ptr(), gt=None, maps=seq.data_ptr(), stream=_lib.current_stream_ptr(img.device), off_r=1, off_c=2)
    assert _lib.load().peanut_mapseq_train_batch(C.byref(d)) == 0
    want = tc.restate(tc.sequences(case)[0], 0, 1, 2, 0, 0, 0.0, case["pad"], case["crop"], case["K"])["img"].astype(np.float32)
    assert _same_bits(img.cpu().numpy()[0], want)


@pytest.mark.parametrize("what", sorted(tc.REFUSALS))
def test_a_refused_call_leaves_the_outputs_untouched(what):
    from peanut_amd import _lib, mapio
    case = tc.OFF_CASES["tall"]
    seq = mapio.to_device(tc.sequences(case)[0])
    img = torch.empty((1, case["C"]) + case["crop"], dtype=torch.float32, device="cuda")
    gt = torch.empty((1, case["K"]) + case["crop"], dtype=torch.uint8, device="cuda")
    img.view(torch.uint8).fill_(0xFF)
    gt.fill_(0xFF)
    edit = dict(tc.REFUSALS[what])
    kw = dict(img=img.data_ptr(), gt=gt.data_ptr(), maps=seq.data_ptr(), stream=_lib.current_stream_ptr(img.device))
    kw.update({k: edit.pop(k) for k in list(edit) if k in kw})
    lib = _lib.load()
    assert lib.peanut_mapseq_train_batch(C.byref(tc.train_desc(**kw, **edit))) == EINVAL, what
    torch.cuda.synchronize()
    assert bool((img.view(torch.uint8) == 0xFF).all()) and bool((gt == 0xFF).all())
    if what == "size":                                         # (the valid descriptor does run: the refusals above are the edits' doing)
        assert lib.peanut_mapseq_train_batch(C.byref(tc.train_desc(**kw))) == 0
        torch.cuda.synchronize()
        assert not bool((img.view(torch.uint8) == 0xFF).all())


def _identity_inputs(S=47, K=6, T=3, B=3):
    from peanut_amd import mapio
    maps = tc.make_sequence(T, 14, (S, S), 21)
    dev = mapio.to_device(maps)
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn((B, K, S, S), generator=g) * 3).cuda()
    return maps, dev, logits


def test_identity_augmentation_gives_the_inputs_the_target_and_the_loss_of_abi_21():
    from peanut_amd import mapio
    S, K, ts = 47, 6, [0, 2, 1]                                 # 2209 cells: three chunks of the loss' partition, the last ragged
    maps, dev, logits = _identity_inputs(S, K)
    aug = mapio.TrainAugment.identity((S, S), seed=3)
    rows = aug.draw(len(ts), (S, S))
    assert not rows["off_r"].any() and not rows["off_c"].any() and not rows["flip"].any() and not rows["rotate"].any()
    img, gt = mapio.train_batch(dev, ts, rows, aug.pad, aug.crop, K=K)
    assert torch.equal(img, mapio.model_input_batch(dev, ts))
    want = np.stack([mapio.target_from_sequence(maps, t, range(4, 4 + K)).transpose(2, 0, 1) for t in ts])
    assert np.array_equal(gt.cpu().numpy(), want) and want.any()
    got, ref = mapio.bce_score_target(logits, gt), mapio.bce_score(logits, dev, ts)
    assert got.dtype == np.float64 and got.shape == (3, K) and _same_bits(got, ref)
    # a rectangular window against the loss in float64 on the host
    lg, tg = logits[:, :, :40, :].contiguous(), gt[:, :, :40, :].contiguous()
    rect = mapio.bce_score_target(lg, tg)
    x = lg.cpu().numpy().astype(np.float64)
    y = (tg.cpu().numpy().astype(np.float32) / np.float32(255)).astype(np.float64)
    cell = (1 - y) * x + np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))
    assert np.abs(rect - cell.sum(axis=(2, 3))).max() <= 64 * 2.0 ** -53 * float(np.sum(np.abs(x) + 1))


def _files(tmp_path, n=2, S=47, T=4):
    files = []
    for k in range(n):
        p = str(tmp_path / f"f{n - k:05d}.npz")                  # written in reverse: the store sorts by name
        np.savez_compressed(p, maps=tc.make_sequence(T, 14, (S, S), 40 + k))
        files.append(p)
    return sorted(files)


def test_store_and_batcher_walk_a_seeded_permutation_of_the_dataset(tmp_path):
    from peanut_amd import mapio
    files = _files(tmp_path)
    t_indices = (0, 2, 1)
    store = mapio.MapStore(str(tmp_path), "cuda:0", t_indices)
    assert store.files == files and store.samples == mapio.dataset_samples(str(tmp_path), t_indices) and len(store) == 6
    full = [mapio.load_map_sequence(f) for f in files]
    assert store.nbytes == sum(4 * m[0].nbytes for m in full)          # three snapshots and the last
    for i, (f, t) in enumerate(store.samples):
        seq, ti = store.sample(i)
        assert np.array_equal(seq[ti].cpu().numpy(), full[files.index(f)][t]) and np.array_equal(seq[-1].cpu().numpy(), full[files.index(f)][-1])
    with pytest.raises(ValueError, match="max_bytes"):
        mapio.MapStore(str(tmp_path), "cuda:0", t_indices, max_bytes=store.nbytes - 1)
    pad, crop, K = (52, 50), (45, 47), 6
    kw = dict(flip_prob=0.5, rotate_prob=0.5, degree=180)
    batcher = mapio.TrainBatcher(store, mapio.TrainAugment(pad, crop, seed=8, **kw), batch=4, seed=5)
    assert len(batcher) == 2
    order_rng, aug = np.random.RandomState(5), mapio.TrainAugment(pad, crop, seed=8, **kw)
    for epoch in range(2):
        order = order_rng.permutation(6)
        batches = list(batcher)
        assert [b["img"].shape[0] for b in batches] == [4, 2] and batcher.epoch == epoch + 1
        for b, lo in zip(batches, (0, 4)):
            assert set(b) == {"img", "gt_semantic_seg", "params"} and b["img"].is_cuda and b["gt_semantic_seg"].is_cuda
            assert b["img"].shape[1:] == (14,) + crop and b["gt_semantic_seg"].shape[1:] == (K,) + crop
            rows = aug.draw(b["img"].shape[0], (47, 47))
            assert rows.tobytes() == b["params"].tobytes()
            for j, i in enumerate(order[lo:lo + 4]):
                f, t = store.samples[i]
                p = rows[j]
                r = tc.restate(full[files.index(f)], t, int(p["off_r"]), int(p["off_c"]), int(p["flip"]), int(p["rotate"]), float(p["angle"]), pad, crop, K)
                if p["rotate"]:
                    assert tc.tie_distance(r["near"]) > tc.TIE_MARGIN
                assert np.abs(b["img"][j].cpu().numpy().astype(np.float64) - r["img"]).max() <= IMG_TOL
                assert np.array_equal(b["gt_semantic_seg"][j].cpu().numpy(), r["gt"])


def test_evaluate_under_the_identity_augmentation_equals_evaluate(tmp_path):
    from types import SimpleNamespace

    from peanut_amd import mapio
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    S, T = 47, 3
    rng = np.random.RandomState(2)
    maps = (rng.uniform(0, 1, (T, 14, S, S)) ** 3 * 255).astype(np.uint8)       # the files of tests/test_mapio_pipeline_gpu.py
    maps[:, 1] *= (rng.uniform(0, 1, (T, S, S)) > 0.6).astype(np.uint8)
    np.savez_compressed(str(tmp_path / "f00002.npz"), maps=maps)
    np.savez_compressed(str(tmp_path / "f00001.npz"), maps=maps[:, :, ::-1].copy())
    model = PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=make_seeded_state_dict(PredCfg(), 0))
    plain = mapio.evaluate(model, str(tmp_path), t_indices=(0, 1, 2))
    same = mapio.evaluate(model, str(tmp_path), t_indices=(0, 1, 2), augment=mapio.TrainAugment.identity((S, S)))
    assert same == plain and plain["n_maps"] == 6
    assert mapio.evaluate(model, str(tmp_path), t_indices=(0, 1, 2), batch=2, augment=mapio.TrainAugment.identity((S, S), seed=1)) == \
        mapio.evaluate(model, str(tmp_path), t_indices=(0, 1, 2), batch=2)
    turned = mapio.evaluate(model, str(tmp_path), t_indices=(0, 1, 2), augment=mapio.TrainAugment((60, 60), (47, 47), seed=0))
    assert turned["n_maps"] == 6 and np.isfinite(turned["loss"]) and turned["loss"] != plain["loss"]
    with pytest.raises(ValueError):
        mapio.evaluate(model, str(tmp_path), window=32, augment=mapio.TrainAugment.identity((S, S)))
