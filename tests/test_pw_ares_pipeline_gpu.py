"""The A-resident GEMM's store pipeline (csrc/conv_pw_ares.hip): a chunk's finished values are held in registers over the
barrier and stored behind the NEXT iteration's weight request, and the bottom wait leaves exactly those stores in flight.
The first unit of a workgroup's range, k-tile 0 of its second unit and the drain are separate code paths, so the shapes
here are the smallest that reach each of them: one unit per workgroup (prologue and drain only), three units per workgroup
with ranges that start and end inside an m-tile, a refill of the A tile in every unit, K = 128 (eight values per chunk),
and the two-level accumulation of the Winograd position GEMMs.  Every case runs with a residual and without, is held bit
for bit to the same handle with the kernel switched off (option pw_ares = 0: the tile-per-workgroup kernels sum in the
same order) and to an fp64 reference; the outputs of the first three also sit between canary rows."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FAMILY = "conv_pw_ares_128x128"
OPTS = {"pw_ares_minunits": 8}          # the kernel's gate is two units per CU; these shapes are smaller on purpose

PW_CASES = {
    # name: (B, H, W, cin, cout)
    "one_unit_per_wg": (1, 32, 32, 256, 256),          # 8 m-tiles x 2 n-tiles = 16 units on 16 workgroups: prologue + drain only
    "three_units_per_wg": (3, 64, 64, 256, 1024),      # 96 x 8 = 768 units over 256 workgroups: ranges start / end inside an m-tile
    "every_unit_refills": (4, 128, 128, 256, 128),     # 512 x 1 units: the A tile is refilled under every unit
    "k128_four_ntiles": (3, 64, 64, 128, 512),         # 96 x 4 = 384 units, K = 128: chunks of eight values
    "k128_two_ntiles": (3, 128, 128, 128, 256),        # 384 x 2 = 768 units
}
OFF_BATCH = {"one_unit_per_wg": 32}     # batch repeats under pw_ares = 0 (see the test)
_cache = {}


def _last_kernel():
    from peanut_amd import _lib
    return _lib.load().peanut_last_conv_kernel().decode()


def _problem(name):
    """Inputs on the device and the fp64 references (with and without the residual), computed once per case."""
    if name not in _cache:
        B, H, W, cin, cout = PW_CASES[name]
        g = torch.Generator().manual_seed(sum(PW_CASES[name]))
        x = torch.randn((B, H, W, cin), generator=g).cuda()
        w = torch.randn((cout, cin, 1, 1), generator=g) * (2.0 / cin) ** 0.5
        scale = torch.rand(cout, generator=g) + 0.5
        shift = torch.randn(cout, generator=g) * 0.1
        res = torch.randn((B, H, W, cout), generator=g).cuda()
        lin = (x.double().reshape(-1, cin) @ w.double().reshape(cout, cin).t().cuda()) * scale.double().cuda() + shift.double().cuda()
        lin = lin.reshape(B, H, W, cout)
        _cache[name] = dict(x=x, w=w, scale=scale, shift=shift, res=res, ref_res=F.relu(lin + res.double()), ref_plain=F.relu(lin))
    return _cache[name]


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("name", list(PW_CASES))
def test_pipelined_stores_against_the_tile_kernels_and_fp64(name, residual):
    from peanut_amd.ops import FusedConv
    pb = _problem(name)
    conv = FusedConv(pb["w"], pb["scale"], pb["shift"], relu=True, options=OPTS)
    res = pb["res"] if residual else None
    y = conv(pb["x"], residual=res)
    assert _last_kernel() == FAMILY, _last_kernel()
    conv.set_option("pw_ares", 0)
    # The tile-per-workgroup kernels cut K into parts when a launch has fewer tiles than the chip has CUs (tail split-K), and then sum
    # in another order.  The rows of a GEMM do not depend on each other, so the 16-tile case is held to the same handle on the same
    # rows inside a batch large enough (512 tiles: two per CU, no tail) for whole-K tiles.
    rep = OFF_BATCH.get(name, 1)
    y_off = conv(pb["x"].repeat(rep, 1, 1, 1), residual=None if res is None else res.repeat(rep, 1, 1, 1))[:pb["x"].shape[0]]
    assert _last_kernel().startswith("conv_pw_glds_128x"), _last_kernel()
    assert torch.equal(y, y_off), float((y - y_off).abs().max())
    ref = pb["ref_res"] if residual else pb["ref_plain"]
    err = (y.double() - ref).abs()
    assert bool((err <= 2e-5 * (1 + ref.abs())).all()), f"max err {err.max().item():.3e}"


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("case", [(1, 32, 32, 256), (2, 32, 32, 128)], ids=["c256", "c128"])
def test_pipelined_stores_under_the_two_level_accumulation(case, residual):
    """A stride-1 3x3 conv in its Winograd form: the grouped position GEMMs (partial sums of 64 channels) run on this kernel.
    Bit for bit against the same handle with the kernel off, and against the direct form of the same conv at the operator
    tolerance tests/test_conv_gpu.py uses for Winograd layers (1.5e-4: the transforms' rounding, not the GEMM's)."""
    from peanut_amd.ops import FusedConv
    B, H, W, c = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn((B, H, W, c), generator=g).cuda()
    w = torch.randn((c, c, 3, 3), generator=g) * (2.0 / (c * 9)) ** 0.5
    shift = torch.randn(c, generator=g) * 0.1
    res = torch.randn((B, H, W, c), generator=g).cuda() if residual else None
    conv = FusedConv(w, None, shift, padding=1, relu=True, options=OPTS)
    y = conv(x, residual=res)
    assert _last_kernel() == FAMILY, _last_kernel()
    conv.set_option("pw_ares", 0)
    y_off = conv(x, residual=res)
    assert _last_kernel() != FAMILY, _last_kernel()
    assert torch.equal(y, y_off), float((y - y_off).abs().max())
    direct = FusedConv(w, None, shift, padding=1, relu=True, conv_algo="direct")(x, residual=res)
    err = (y - direct).abs()
    assert bool((err <= 1.5e-4 * (1 + direct.abs())).all()), f"max err {err.max().item():.3e}"


@pytest.mark.parametrize("name", ["one_unit_per_wg", "three_units_per_wg", "every_unit_refills"])
def test_no_store_lands_outside_the_tensor_and_none_is_lost(name):
    """The output sits inside a larger buffer between canary rows: they come back untouched (a held chunk stored through the
    next unit's pointer, or a drain that runs one chunk too far, would hit them), and a second run into a NaN-filled output
    writes every element again."""
    from peanut_amd import _lib
    from peanut_amd.ops import FusedConv
    B, H, W, cin, cout = PW_CASES[name]
    pb = _problem(name)
    conv = FusedConv(pb["w"], pb["scale"], pb["shift"], relu=True, options=OPTS)
    want = conv(pb["x"], residual=pb["res"])
    assert _last_kernel() == FAMILY, _last_kernel()
    M, guard = B * H * W, 256
    buf = torch.full((M + 2 * guard, cout), -12345.0, device="cuda")
    y = buf[guard:guard + M]

    def run():
        with torch.cuda.device(pb["x"].device):
            _lib.check(conv._lib.peanut_conv_forward(conv._h, pb["x"].data_ptr(), None, cin, pb["res"].data_ptr(), y.data_ptr(), B, H, W,
                                                     _lib.current_stream_ptr(pb["x"].device)), "peanut_conv_forward")
        assert _last_kernel() == FAMILY, _last_kernel()

    run()
    assert torch.equal(y.reshape(want.shape), want)
    assert bool((buf[:guard] == -12345.0).all()) and bool((buf[guard + M:] == -12345.0).all())
    y.fill_(float("nan"))
    run()
    assert not bool(torch.isnan(y).any())
    assert torch.equal(y.reshape(want.shape), want)
    assert bool((buf[:guard] == -12345.0).all()) and bool((buf[guard + M:] == -12345.0).all())
