"""Map datasets on the device (csrc/mapio.hip, ABI 21) against the NumPy statements of the reference: the snapshot
(collect_maps.py:81-82), the filter's sums (:86), the model input (train_prediction_model.py:66-68) and the loss (:173-184 on the
target of :85-89)."""
import math

import numpy as np
import pytest
import torch

from workspace_cases import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- encode -----------------------------------------------------------------------------------------------------------------
def _edge_values():
    """For every k in 0..255 the fp32 values k/255, one ulp below and one ulp above; then 0, -0.0, the smallest denormal and 1.
    On all of them ``(x * 255).astype(np.uint8)`` is defined: the products lie in (-1, 256)."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    v = np.stack([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))], axis=1).reshape(-1)
    v = np.concatenate([v, np.array([0.0, -0.0, np.float32(1e-45), 1.0], np.float32)]).astype(np.float32)
    prod = v * np.float32(255)
    assert prod.min() > -1 and prod.max() < 256
    return v


def _edge_map(shape, shift=0):
    v = _edge_values()
    n = int(np.prod(shape))
    return v[(np.arange(n) + shift) % v.size].reshape(shape)


def _host(x):
    return (x * 255).astype(np.uint8)


def _encode(ts, **kw):
    from peanut_amd import mapio
    out, sums = mapio.encode_maps_device(ts, **kw)
    return [o.cpu() for o in out], sums.cpu().tolist()


def test_encode_values_at_every_byte_boundary():
    from peanut_amd import mapio
    v = _edge_values()
    assert np.array_equal(_host(v[:768:3]), np.arange(256))                                      # k/255 -> k
    assert np.array_equal(_host(v[1:768:3]), np.maximum(np.arange(256) - 1, 0))                  # one ulp below -> k - 1
    assert np.array_equal(_host(v[2:768:3]), np.arange(256))                                     # one ulp above -> k
    x = _edge_map((14, 24, 24))                                                                  # 8064 cells: ten cycles of the 772 values
    want = torch.from_numpy(_host(x))
    (dev_out,), sums = _encode([torch.from_numpy(x).to(DEV)])                                    # the kernel
    assert torch.equal(dev_out, want)
    assert sums == [[int(want[4:].sum(dtype=torch.int64)), int(want[1].sum(dtype=torch.int64))]]
    # encode_map of a HIP tensor keeps the host route: only its return type and its agreement with the kernel
    got = mapio.encode_map(torch.from_numpy(x).to(DEV))
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and torch.equal(torch.from_numpy(got), dev_out)
    with pytest.raises(ValueError):
        mapio.encode_maps_device([x])                                                            # a NumPy array is no HIP tensor


@pytest.mark.parametrize("shape", [(5, 1, 1), (14, 47, 47), (14, 96, 96), (25, 33, 65)])
def test_encode_shapes_and_prefilled_outputs(shape):
    """Rows that are no multiple of four floats, a plane of one cell; dst and the sums hold 0xFF before the call."""
    x = _edge_map(shape, shift=shape[0] + shape[2])
    want = _host(x)
    dst = torch.full(shape, 0xFF, dtype=torch.uint8, device=DEV)
    sums = torch.full((1, 2), -1, dtype=torch.int64, device=DEV)
    (got,), s = _encode([torch.from_numpy(x).to(DEV)], out=[dst], sums=sums)
    assert torch.equal(got, torch.from_numpy(want))
    assert s == [[int(np.sum(want[4:])), int(np.sum(want[1]))]]


@pytest.mark.parametrize("rows,cols", [(slice(3, 50), slice(5, 52)), (slice(4, 52), slice(8, 56)), (slice(0, 48), slice(2, 50))])
def test_encode_reads_a_view_where_it_lies(rows, cols):
    """47 x 47 at an odd offset (the scalar path), 48 x 48 at a 32-byte offset (16-byte loads over strided rows), 48 x 48 at an
    8-byte offset (rows of four floats whose addresses do not allow them)."""
    big = torch.from_numpy(_edge_map((14, 64, 64), shift=7)).to(DEV)
    view = big[:, rows, cols]
    assert not view.is_contiguous()
    (a,), sa = _encode([view])
    (b,), sb = _encode([view.contiguous()])
    assert torch.equal(a, b) and sa == sb
    assert torch.equal(a, torch.from_numpy(_host(view.cpu().numpy())))


def test_encode_batches_equal_single_calls():
    from peanut_amd import mapio
    rng = np.random.RandomState(5)
    maps = [torch.from_numpy(rng.uniform(0, 1, (14, 47, 47)).astype(np.float32) * (rng.uniform(0, 1, (14, 1, 1)) > 0.3)).float().to(DEV)
            for _ in range(16)]
    maps[3] = maps[3].new_zeros((14, 64, 64))[:, 3:50, 5:52].copy_(maps[3])                     # one view among them
    single = [_encode([m]) for m in maps]
    for E in (1, 2, 3, 16):
        outs, sums = _encode(maps[:E])
        for e in range(E):
            assert torch.equal(outs[e], single[e][0][0]), (E, e)
            assert sums[e] == single[e][1][0], (E, e)
    with pytest.raises(ValueError):
        mapio.encode_maps_device(maps + [maps[0]])                                               # E = 17


def test_encode_sums_pass_32_bits():
    """960 x 960 x 25 of ones (the project's config 5): 21 * 921600 * 255 = 4 935 168 000 > 2^32."""
    x = torch.ones((25, 960, 960), device=DEV)
    out, sums = _encode([x])
    assert sums == [[21 * 921600 * 255, 921600 * 255]] and sums[0][0] > 2 ** 32
    assert bool((out[0] == 255).all())


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _sequence(T=3, C=14, W=47, H=47, seed=0):
    rng = np.random.RandomState(seed)
    maps = rng.randint(0, 256, (T, C, W, H)).astype(np.uint8)
    maps[0, 0].reshape(-1)[:256] = np.arange(256)                     # every byte value is there
    maps[:, 1] *= (rng.uniform(0, 1, (T, W, H)) > 0.5).astype(np.uint8)      # explored: about half the cells
    return maps


def _host_input(maps, t, x1, y1, S):
    return maps[t, :, x1:x1 + S, y1:y1 + S].astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("W", [47, 48])
def test_inputs_equal_the_numpy_expression(W):
    from peanut_amd import mapio
    maps = _sequence(W=W, H=W)
    dev = mapio.to_device(maps, DEV)
    T = maps.shape[0]
    assert set(np.unique(maps[0, 0])) == set(range(256))
    whole = mapio.model_input_batch(dev, [0, T - 1])
    for b, t in enumerate((0, T - 1)):
        assert torch.equal(whole[b].cpu(), torch.from_numpy(_host_input(maps, t, 0, 0, W)))
        assert torch.equal(whole[b:b + 1].cpu(), mapio.model_input(maps, t))
    S = 16
    corners = [(0, 0), (0, W - S), (W - S, 0), (W - S, W - S)]
    ts = [0, 1, T - 1, 1]
    got = mapio.model_input_batch(dev, ts, window=S, origin=corners)             # one triple per sample
    for b, (t, (x1, y1)) in enumerate(zip(ts, corners)):
        assert torch.equal(got[b].cpu(), torch.from_numpy(_host_input(maps, t, x1, y1, S))), b
    aligned = mapio.model_input_batch(dev, [2, 0], window=S, origin=[(5, 8), (31, 28)])   # columns at multiples of four
    assert torch.equal(aligned[0].cpu(), torch.from_numpy(_host_input(maps, 2, 5, 8, S)))
    assert torch.equal(aligned[1].cpu(), torch.from_numpy(_host_input(maps, 0, 31, 28, S)))
    centre = mapio.model_input_batch(dev, 1, window=S)                            # Agent_State._prediction_crop's window
    o = W // 2 - S // 2
    assert torch.equal(centre[0].cpu(), torch.from_numpy(_host_input(maps, 1, o, o, S)))


def test_inputs_refuse_a_window_over_the_edge_and_enqueue_nothing():
    from peanut_amd import mapio
    maps = _sequence()
    dev = mapio.to_device(maps, DEV)
    out = torch.full((1, 14, 16, 16), 7.0, device=DEV)
    for org in [(32, 0), (0, 32), (-1, 0)]:
        with pytest.raises(ValueError):
            mapio.model_input_batch(dev, 0, window=16, origin=org, out=out)
    for t in (3, -1):
        with pytest.raises(ValueError):
            mapio.model_input_batch(dev, t, window=16, origin=(0, 0), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the loss ---------------------------------------------------------------------------------------------------------------
LOGITS = np.array([0.0, 1e-30, -1e-30, 0.5, -0.5, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4], np.float32)
S_BCE, K_BCE = 96, 6


@pytest.fixture(scope="module")
def bce_case():
    """One 96 x 96 sequence whose last snapshot holds, in channel 4 + k, all 256 bytes against the 13 logits with the explored
    byte of snapshot 0 off and on (13 * 256 * 2 = 6656 <= 9216 cells); snapshot 1 has another explored mask.  Five samples; the
    float64 reference per (b, k), summed with math.fsum; the fp32 statement of the reference on the CPU, summed in float64."""
    import torch.nn.functional as F
    from peanut_amd import mapio
    T, C, S, K = 3, 14, S_BCE, K_BCE
    n = np.arange(S * S)
    rng = np.random.RandomState(11)
    maps = rng.randint(0, 256, (T, C, S, S)).astype(np.uint8)
    maps[0, 1] = (((n // (13 * 256)) % 2) * 200).astype(np.uint8).reshape(S, S)
    maps[1, 1] = (rng.uniform(0, 1, (S, S)) > 0.5) * rng.randint(1, 256, (S, S))
    logits = np.empty((5, K, S, S), np.float32)
    for k in range(K):
        maps[T - 1, 4 + k] = (((n + 17 * k) // 13) % 256).astype(np.uint8).reshape(S, S)
    for b in range(5):
        for k in range(K):
            logits[b, k] = LOGITS[(n + 3 * b + 5 * k) % 13].reshape(S, S)
    logits[0] = np.stack([LOGITS[n % 13].reshape(S, S)] * K)                   # sample 0: the plain cycle on every channel
    t_idx = [0, 1, 0, 2, 1]
    ref64 = np.empty((5, K))
    ref32 = np.empty((5, K))
    bound = np.empty((5, K))
    for b, t in enumerate(t_idx):
        tgt = mapio.target_from_sequence(maps, t, range(4, 4 + K)).transpose(2, 0, 1)        # [K,S,S] bytes (:85-89)
        assert tgt.max() <= 255 and tgt.min() >= 0
        y32 = tgt.astype(np.float32) / np.float32(255)
        x, y = logits[b].astype(np.float64), y32.astype(np.float64)
        cell = (1 - y) * x + np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))
        l32 = F.binary_cross_entropy_with_logits(torch.from_numpy(logits[b]), torch.from_numpy(tgt.astype(np.float32)) / 255.,
                                                 reduction='none')
        for k in range(K):
            ref64[b, k] = math.fsum(cell[k].reshape(-1).tolist())
            ref32[b, k] = float(l32[k].double().sum())
            bound[b, k] = 64 * 2.0 ** -53 * float(np.sum(np.abs(x[k]) + 1))
    # every (logit, byte, explored) combination is there: sample 0, channel 4
    last, expl = maps[T - 1, 4].reshape(-1), maps[0, 1].reshape(-1)
    assert len({(int(i % 13), int(last[i]), int(expl[i] != 0)) for i in range(6656)}) == 13 * 256 * 2
    return dict(maps=maps, dev=mapio.to_device(maps, DEV), logits=torch.from_numpy(logits).to(DEV), t_idx=t_idx,
                ref64=ref64, ref32=ref32, bound=bound)


def test_bce_against_the_float64_reference_and_the_reference_statement(bce_case):
    from peanut_amd import mapio
    c = bce_case
    got = mapio.bce_score(c["logits"], c["dev"], c["t_idx"])
    assert got.dtype == np.float64 and got.shape == (5, K_BCE)
    err64 = np.abs(got - c["ref64"])
    err32 = np.abs(got - c["ref32"])
    gap = np.abs(c["ref32"] - c["ref64"])
    print(f"bce: max |dev - ref64| = {err64.max():.3e} (bound {c['bound'].min():.3e}..{c['bound'].max():.3e}), "
          f"max |dev - ref32| = {err32.max():.3e}, max |ref32 - ref64| = {gap.max():.3e}")
    assert bool((err64 <= c["bound"]).all()), (err64 / c["bound"]).max()
    assert bool((err32 <= gap + c["bound"]).all())


def test_bce_windows_match_the_reference_too(bce_case):
    """A 47 x 47 window at an odd origin (cells that are no multiple of the chunk) of the same sequence."""
    from peanut_amd import mapio
    c = bce_case
    maps, S, (x1, y1), t = c["maps"], 47, (13, 30), 1
    lg = c["logits"][1:2, :, :S, :S].contiguous()
    got = mapio.bce_score(lg, c["dev"], [t], window=S, origin=(x1, y1))
    tgt = mapio.target_from_sequence(maps, t, range(4, 4 + K_BCE)).transpose(2, 0, 1)[:, x1:x1 + S, y1:y1 + S]
    x = lg[0].cpu().numpy().astype(np.float64)
    y = (tgt.astype(np.float32) / np.float32(255)).astype(np.float64)
    cell = (1 - y) * x + np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))
    for k in range(K_BCE):
        ref = math.fsum(cell[k].reshape(-1).tolist())
        assert abs(got[0, k] - ref) <= 64 * 2.0 ** -53 * float(np.sum(np.abs(x[k]) + 1)), k


def test_bce_bits_do_not_depend_on_the_batch_the_slot_or_the_run(bce_case):
    from peanut_amd import mapio
    c = bce_case
    all5 = mapio.bce_score(c["logits"], c["dev"], c["t_idx"])
    again = mapio.bce_score(c["logits"], c["dev"], c["t_idx"])
    assert all5.tobytes() == again.tobytes()
    alone = mapio.bce_score(c["logits"][3:4].contiguous(), c["dev"], [c["t_idx"][3]])          # slot 0 of B = 1
    assert alone[0].tobytes() == all5[3].tobytes()                                             # slot 3 of B = 5
    order = [3, 0, 4]
    mixed = mapio.bce_score(c["logits"][order].contiguous(), c["dev"], [c["t_idx"][b] for b in order])
    assert mixed.tobytes() == all5[order].tobytes()


def test_results_do_not_depend_on_what_scratch_held(bce_case):
    """The three calls with the library's own allocations poisoned (0xFF: NaN as a double) give the bits they give without."""
    from peanut_amd import mapio
    c = bce_case
    x = torch.from_numpy(_edge_map((14, 47, 47))).to(DEV)
    clean = (_encode([x, x]), mapio.model_input_batch(c["dev"], [0, 2], window=47).cpu(),
             mapio.bce_score(torch.cat([c["logits"], c["logits"]]), c["dev"], c["t_idx"] * 2))
    with poisoned():
        lg = torch.cat([c["logits"]] * 3)                                                      # more partial sums than any call before
        big = mapio.bce_score(lg, c["dev"], c["t_idx"] * 3)
        dirty = (_encode([x, x]), mapio.model_input_batch(c["dev"], [0, 2], window=47).cpu(),
                 mapio.bce_score(torch.cat([c["logits"], c["logits"]]), c["dev"], c["t_idx"] * 2))
    assert torch.equal(clean[0][0][0], dirty[0][0][0]) and clean[0][1] == dirty[0][1]
    assert torch.equal(clean[1].view(torch.int32), dirty[1].view(torch.int32))
    assert clean[2].tobytes() == dirty[2].tobytes()
    assert big[:10].tobytes() == clean[2].tobytes() and np.isfinite(big).all()
