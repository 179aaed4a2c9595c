"""The conv / GEMM kernels behind the NON-default value of the tuning options (csrc/options.h) no other test sets: every case
creates its handle with ``options=`` (or flips a run-time key with ``set_option``), asserts the kernel family that ran
(peanut_last_conv_kernel) and holds the result to ``torch.nn.functional.conv2d`` on float64 CPU tensors with the epilogue
(scale, shift, residual, ReLU) in float64, at the tolerance the neighbouring tests of tests/test_conv_gpu.py use for the same
operator and mode: 2e-5 * (1 + |ref|) for the fp32 pointwise and direct kernels, RS_TOL for the emulated modes.  Every case prints
its worst error relative to 1 + |ref|.

Bit-for-bit equality with the default-option handle is asserted exactly where the code shows that the option cannot change the
order of any sum (it only moves WHEN or WHERE a tile is computed); where it changes which tiles are cut along K, how K is cut or
the k-tile width, both results are held to the reference and their distance to the operator tolerance.  Each docstring says which
of the two holds and why.  The shapes are small: the large-tile gates are lowered per handle, as WIDE_OPTS / WP_OPTS / P256P_OPTS
do in tests/test_conv_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from test_conv_gpu import P256P_OPTS, RS_TAG, RS_TOL, WP_OPTS, _last_kernel

pytestmark = pytest.mark.gpu

FP32_TOL = 2e-5
W256_OPTS = {"pw256w_mink": 256, "pw256w_mintiles": 1, "pw256wp_mink": 0}      # the 256 x 256 two-stage kernel for a handful of tiles
ARES_OPTS = {"pw_ares_minunits": 8}                                             # the A-resident kernel from 8 units on (its launcher's floor)
RS256_OPTS = {"rs256_mink": 64, "rs256_mintiles": 1, "rs64_maxtiles": 0}        # gemm_rs 256 x 256 for a handful of tiles


def _make_problem(B, H, W, cin, cout, k=1, dil=1, relu=True, residual=True):
    """Seeded operator + its float64 reference: (x NHWC on the device, OIHW weight, scale, shift, residual NHWC on the device or
    None, reference NHWC float64 on the host)."""
    g = torch.Generator().manual_seed(1000 * cin + cout + 7 * H + W + k)
    x = torch.randn((B, cin, H, W), generator=g)
    w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    pad = dil * (k // 2)
    ref = F.conv2d(x.double(), w.double(), None, padding=pad, dilation=dil) * scale.double()[None, :, None, None] \
        + shift.double()[None, :, None, None]
    res = None
    if residual:
        res = torch.randn(tuple(ref.shape), generator=g)
        ref = ref + res.double()
    if relu:
        ref = F.relu(ref)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    rd = None if res is None else res.permute(0, 2, 3, 1).contiguous().cuda()
    return xd, w, scale, shift, rd, ref.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def problems():
    """problems(B, H, W, cin, cout, ...) -> the operator of that shape and its reference, made once per module and shared by the
    cases that use the shape; nothing is written to them.  The large ones (the 512-tile launches) are not kept."""
    made = {}

    def get(*args, **kw):
        key = (args, tuple(sorted(kw.items())))
        if key in made:
            return made[key]
        prob = _make_problem(*args, **kw)
        if prob[5].numel() <= 4 << 20:
            made[key] = prob
        return prob
    yield get
    made.clear()


def _conv(prob, k=1, dil=1, relu=True, precision="fp32", conv_algo="auto", options=None):
    from peanut_amd.ops import FusedConv
    _, w, scale, shift, _, _ = prob
    return FusedConv(w, scale, shift, padding=dil * (k // 2), dilation=dil, relu=relu, precision=precision, conv_algo=conv_algo,
                     options=options)


def _run(conv, prob, family, c1=None):
    """One forward (two sources when c1 is given: the input split after c1 channels), the family asserted, run twice (deterministic)."""
    xd, _, _, _, rd, _ = prob
    if c1 is None:
        y = conv(xd, residual=rd)
        again = conv(xd, residual=rd)
    else:
        xa, xb = xd[..., :c1].contiguous(), xd[..., c1:].contiguous()
        y = conv(xa, x2=xb, residual=rd)
        again = conv(xa, x2=xb, residual=rd)
    assert _last_kernel() == family, _last_kernel()
    assert torch.equal(y, again)
    return y


def _rel_err(y, ref):
    return float(((y.cpu().double() - ref).abs() / (1 + ref.abs())).max())


def _hold(y, prob, tol, what):
    err = _rel_err(y, prob[5])
    print(f"{what}: worst |y - ref| / (1 + |ref|) = {err:.3e} (bound {tol:.1e})")
    assert err <= tol, f"{what}: {err:.3e}"
    return err


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _mutual(a, b, prob, tol, what):
    """Two results of one operator whose sums run in another order: within the operator tolerance of each other."""
    d = float(((a - b).abs().cpu().double() / (1 + prob[5].abs())).max())
    print(f"{what}: worst distance between the two settings / (1 + |ref|) = {d:.3e}")
    assert d <= tol, f"{what}: {d:.3e}"


# ---- nchunk: the chunked tile order of tile_to_mn (csrc/conv_common.h) ----
# (B, H, W, cin, cout, k): M = 399 rows (ragged last m-tile) unless noted.  With the default nchunk = 8 these have a last chunk of
# fewer than eight n-tiles -- the remainder branch no layer of the project's own nets reaches (2, 4, 8 or 16 n-tiles).
NCHUNK_DEFAULT_CASES = [
    ((1, 21, 19, 160, 1152, 1), "conv_pw_glds_128x64"),       # 128-wide packed, <= 256 channels and few tiles: 64-wide tiles, 18 n-tiles (remainder 2)
    ((1, 21, 19, 160, 1280, 1), "conv_pw_glds_128x64"),       # 20 n-tiles (remainder 4)
    ((1, 21, 19, 288, 1152, 1), "conv_pw_glds_128x128"),      # 9 n-tiles of 128 (remainder 1); 9 k-tiles: the tail plan cuts every tile in two
    ((1, 21, 19, 288, 1280, 1), "conv_pw_glds_128x128"),      # 10 n-tiles (remainder 2)
    ((2, 25, 25, 512, 1152, 1), "conv_pw_glds_128x128"),      # 10 x 9 tiles of 16 k-tiles: split along K (test_split_model... shows it is)
    ((1, 21, 19, 64, 640, 1), "conv_pw_glds_128x64"),         # 64-wide packed: 10 n-tiles (remainder 2)
    ((1, 12, 12, 32, 1152, 3), "conv_igemm_128x64x32"),       # 3x3, 18 n-tiles, 9 k-tiles: split in two
]


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case,family", NCHUNK_DEFAULT_CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else c)
def test_nchunk_remainder_branch_at_default_options(problems, case, family, residual):
    """More than eight n-tiles, not a multiple of eight: tile_to_mn's last, narrower chunk (conv_common.h) at DEFAULT options, on the
    fp32 128-wide and 64-wide pointwise kernels and conv_igemm, without and with a residual.  Where the launch cuts its tiles along K
    conv_splitk_reduce_kernel decodes the same tiles through the same function and adds the residual itself.  By plan_tail_split's
    cost model that is every case of nine or more k-tiles here, but these cases do not assert it and they never mix whole and cut
    tiles: test_split_model_0_plans_the_tail_by_slots shows the cut for the 2 x 25 x 25 x 512 x 1152 shape, and
    test_nchunk_remainder_branch_with_whole_and_cut_tiles runs the chunked order with both kinds of tile in one launch.

    Against nchunk = 0 (n fastest over all n-tiles) on the same handle: bit for bit.  These launches have fewer tiles than resident
    workgroup slots, so either every tile is a tail tile or none is (launch_with_tail_split: t = T mod S = T): the order decides
    which workgroup computes a tile, not how its sum is formed."""
    B, H, W, cin, cout, k = case
    prob = problems(B, H, W, cin, cout, k=k, residual=residual)
    conv = _conv(prob, k=k, conv_algo="direct")
    y = _run(conv, prob, family)
    _hold(y, prob, FP32_TOL, f"nchunk=8 {family} {case} residual={residual}")
    conv.set_option("nchunk", 0)
    y0 = _run(conv, prob, family)
    assert _same_bits(y, y0), f"differs from the plain order in {(y != y0).sum().item()} values"


@pytest.mark.parametrize("nchunk", [8, 3])
def test_nchunk_remainder_branch_with_whole_and_cut_tiles(problems, nchunk):
    """More tiles than resident workgroup slots: 60 x 9 = 540 tiles of 128 x 128 (M = 7 650, ragged) over 512 slots leave 28 tail tiles,
    which the plan cuts in two along K (9 k-tiles) -- whole tiles and split parts in one launch, n_full > 0, and the reduce kernel
    decoding tiles 512..539 of the chunked order.  Under nchunk = 8 those are the narrow last chunk (n-tile 8, m-tiles 32..59); under
    nchunk = 3 the last chunk of three; under the plain order m-tiles 56..59.  WHICH tiles are cut differs between the orders, so
    the results may differ where the sums were cut: each is held to the reference and the two to the operator tolerance of each
    other, and that they do differ in some bit is what shows that tiles were cut at all and that the chunked order chose others."""
    prob = problems(3, 50, 51, 288, 1152)
    conv = _conv(prob, options={"nchunk": nchunk})
    y = _run(conv, prob, "conv_pw_glds_128x128")
    _hold(y, prob, FP32_TOL, f"nchunk={nchunk}, 540 tiles")
    conv.set_option("nchunk", 0)
    y0 = _run(conv, prob, "conv_pw_glds_128x128")
    _hold(y0, prob, FP32_TOL, "nchunk=0, 540 tiles")
    assert not _same_bits(y, y0), "the chunked and the plain order cut the same tiles: no whole / cut mix at this shape"
    _mutual(y, y0, prob, FP32_TOL, f"nchunk {nchunk} / 0 with a 28-tile tail")


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case,family,options", [
    ((1, 21, 19, 160, 1152, 1), "gemm_rs6_64x64", None),                           # 7 x 18 tiles of 64 x 64, 10 k-tiles of 16: split
    ((1, 21, 19, 160, 1280, 1), "gemm_rs6_64x64", None),
    ((1, 21, 19, 64, 640, 1), "gemm_rs6_64x64", None),                             # 64-wide packed
    ((1, 21, 19, 288, 1152, 1), "gemm_rs6_128x128", {"rs64_maxtiles": 0}),         # 4 x 9 tiles of 128 x 128 (the 64 x 64 gate closed)
    ((1, 12, 12, 32, 1152, 3), "conv_rs6_128x128", None),                          # conv_rs.hip: 9 n-tiles
], ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else (c if isinstance(c, str) else "opts"))
def test_nchunk_remainder_branch_in_bf16x6(problems, case, family, options, residual):
    """The same shapes through gemm_rs.hip / conv_rs.hip (bf16x6), whose launches go through launch_with_tail_split as well; the
    64 x 64 kernel walks 18 / 20 / 10 n-tiles.  Bit for bit against nchunk = 0, for the reason given above."""
    B, H, W, cin, cout, k = case
    prob = problems(B, H, W, cin, cout, k=k, residual=residual)
    conv = _conv(prob, k=k, precision="bf16x6", conv_algo="direct", options=options)
    y = _run(conv, prob, family)
    _hold(y, prob, RS_TOL["bf16x6"], f"nchunk=8 {family} {case} residual={residual}")
    conv.set_option("nchunk", 0)
    assert _same_bits(y, _run(conv, prob, family))


NCHUNK_FAMILIES = [
    # family, (B, H, W, cin, cout, k), precision, options: cout = 1024 is eight 128-wide n-tiles -- two chunks of three and one of
    # two under nchunk = 3 -- or sixteen 64-wide ones (five chunks and one tile) or four 256-wide ones (one chunk and one tile)
    ("conv_pw_glds_128x128", (1, 21, 19, 288, 1024, 1), "fp32", {}),
    ("conv_pw_glds_128x64", (1, 21, 19, 160, 1024, 1), "fp32", {}),
    ("conv_pw_glds_128x64", (1, 21, 19, 64, 1024, 1), "fp32", {}),
    ("conv_pw_glds_256x128", (1, 21, 19, 1024, 1024, 1), "fp32", {"pw256_mintiles": 1}),
    ("conv_pw_glds_256x256", (1, 21, 19, 512, 1024, 1), "fp32", W256_OPTS),
    ("conv_igemm_128x64x32", (1, 12, 12, 32, 1024, 3), "fp32", {}),
    ("conv_igemm_128x128x32", (1, 12, 12, 320, 1024, 3), "fp32", {}),
    ("gemm_rs6_64x64", (1, 21, 19, 160, 1024, 1), "bf16x6", {}),
    ("gemm_rs6_128x128", (1, 21, 19, 288, 1024, 1), "bf16x6", {"rs64_maxtiles": 0}),
    ("gemm_rs6_256x256", (1, 21, 19, 160, 1024, 1), "bf16x6", RS256_OPTS),
    ("conv_rs6_128x128", (1, 12, 12, 32, 1024, 3), "bf16x6", {}),
    ("conv_pw_glds_256x128p", (1, 32, 32, 512, 1024, 1), "fp32", P256P_OPTS),          # 4 x 8 tiles, all in split parts
    ("conv_pw_glds_256x128p", (1, 40, 25, 512, 1024, 1), "fp32", P256P_OPTS),          # M = 1000: the RAGGED variant
    ("conv_pw_glds_256x256p", (1, 32, 32, 512, 2048, 1), "fp32", WP_OPTS),             # 4 x 8 tiles of 256 x 256
]


@pytest.mark.parametrize("nchunk", [3, 0])
@pytest.mark.parametrize("family,case,precision,options", NCHUNK_FAMILIES,
                         ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else (c if isinstance(c, str) else "opts"))
def test_nchunk_3_and_0_on_every_kernel_that_reads_it(problems, family, case, precision, options, nchunk):
    """nchunk = 3 (whole chunks and a narrower last one at every width of n-tile) and nchunk = 0 (the plain order) on every kernel
    whose launcher reads the option: the users of launch_with_tail_split (conv_pw.hip's three tile shapes and the 256-row kernels,
    conv_igemm, gemm_rs, conv_rs) and the two persistent kernels (conv_pw256p.hip, conv_pw256wp.hip), with a residual, so that a
    split tile's residual is added by the reduce kernel, which decodes the tile through tile_to_mn as well.

    Bit for bit against the default order on the same handle.  The option only renumbers tiles; which tiles are cut along K could
    change only if some were whole and some cut, and every launch here has fewer tiles than workgroup slots (all cut or none) --
    the persistent kernels included: 32 tiles over one workgroup per CU are all dealt out in parts."""
    B, H, W, cin, cout, k = case
    prob = problems(B, H, W, cin, cout, k=k)
    conv = _conv(prob, k=k, precision=precision, conv_algo="direct", options=options)
    y8 = _run(conv, prob, family)
    conv.set_option("nchunk", nchunk)
    y = _run(conv, prob, family)
    tol = FP32_TOL if precision == "fp32" else RS_TOL[precision]
    _hold(y, prob, tol, f"nchunk={nchunk} {family} {case}")
    _hold(y8, prob, tol, f"nchunk=8 {family} {case}")
    assert _same_bits(y, y8), f"differs from the default order in {(y != y8).sum().item()} values"


# ---- pw256_phase: the five kernels whose two waves per SIMD request their LDS-DMA pieces half an iteration apart ----
PHASE_KERNELS = [
    ("conv_pw_glds_256x128", (1, 21, 19, 1024, 256), {"pw256_mintiles": 1}),
    ("conv_pw_glds_256x256", (1, 21, 19, 512, 512), W256_OPTS),
    ("conv_pw_ares_128x128", (1, 16, 24, 256, 1024), ARES_OPTS),                  # 3 x 8 units on 24 workgroups
    ("conv_pw_glds_256x128p", (1, 32, 32, 512, 1024), P256P_OPTS),
    ("conv_pw_glds_256x256p", (1, 32, 32, 512, 512), WP_OPTS),
]


@pytest.mark.parametrize("family,case,options", PHASE_KERNELS, ids=lambda c: c if isinstance(c, str) else ("x".join(map(str, c)) if isinstance(c, tuple) else "opts"))
def test_pw256_phase_0_on_the_five_kernels_that_read_it(problems, family, case, options):
    """pw256_phase = 0: waves 4-7 issue their LDS-DMA requests at the top of the iteration like waves 0-3, not after their first
    MFMAs.  The flag moves the requests of a k-tile inside the iteration before the one that reads it (`late` in each kernel);
    fragments, MFMA order and epilogue are the same code, so the result must equal the default's bit for bit -- nothing observable
    changes but the timing, and the case holds both settings to the reference."""
    prob = problems(*case)
    conv = _conv(prob, options=options)
    y1 = _run(conv, prob, family)
    conv.set_option("pw256_phase", 0)
    y0 = _run(conv, prob, family)
    _hold(y0, prob, FP32_TOL, f"pw256_phase=0 {family} {case}")
    _hold(y1, prob, FP32_TOL, f"pw256_phase=1 {family} {case}")
    assert _same_bits(y0, y1), f"{(y0 != y1).sum().item()} values differ"


# (pw256_skip_pad acts only where the caller tells the launch how many rows of a weight group hold data -- ConvArgs::group_valid_rows,
# which the prediction planner alone sets: tests/test_option_policy_gpu.py runs it there.)


# ---- pw256p_order / pw256wp_stagger: the persistent kernels' item order and start times ----
@pytest.mark.parametrize("family,case,options", [
    ("conv_pw_glds_256x128p", (4, 64, 64, 256, 1024), P256P_OPTS),      # 64 x 8 = 512 tiles: two whole tiles per workgroup, no tail
    ("conv_pw_glds_256x128p", (1, 144, 128, 256, 1024), P256P_OPTS),    # 576 tiles: two each + 64 tail tiles in parts
    ("conv_pw_glds_256x256p", (4, 64, 64, 64, 2048), WP_OPTS),          # 512 tiles of 256 x 256, no tail
    ("conv_pw_glds_256x256p", (1, 144, 128, 64, 2048), WP_OPTS),        # 576 tiles: a 64-tile tail
], ids=lambda c: c if isinstance(c, str) else ("x".join(map(str, c)) if isinstance(c, tuple) else "opts"))
def test_pw256p_order_0_on_both_persistent_kernels(problems, family, case, options):
    """pw256p_order = 0: every workgroup walks one contiguous run of whole tiles (tile = lw * nf + i) instead of the interleaved
    runs of an XCD's workgroups.  The order matters from two whole tiles per workgroup on (nf >= 2: 512 tiles over the 256 CUs;
    with one the two formulas coincide), hence these sizes; K is the smallest each kernel takes.  Whole tiles stay whole and tail
    tiles stay the last T mod G tiles under either order, so no sum changes: bit for bit equal to the default, without and with a
    tail."""
    B, H, W, cin, cout = case
    opts = dict(options)
    if cin <= 128:
        opts["pw_bn64_maxk"] = 0                  # pack this narrow layer 128 wide (the kernel reads 128-wide packed weights)
    prob = problems(B, H, W, cin, cout)
    conv = _conv(prob, options=opts)
    y1 = _run(conv, prob, family)
    conv.set_option("pw256p_order", 0)
    y0 = _run(conv, prob, family)
    _hold(y0, prob, FP32_TOL, f"pw256p_order=0 {family} {case}")
    _hold(y1, prob, FP32_TOL, f"pw256p_order=1 {family} {case}")
    assert _same_bits(y0, y1), f"{(y0 != y1).sum().item()} values differ"


@pytest.mark.parametrize("stagger", [1, 7])
def test_pw256wp_stagger_only_delays_the_start(problems, stagger):
    """pw256wp_stagger > 0: a workgroup sleeps up to `stagger` slots of ~3.4 us before its first request.  Nothing else reads the
    value, so the result equals the unstaggered one bit for bit (the option only reschedules); 8 tiles in split parts and a residual."""
    prob = problems(1, 32, 32, 512, 512)
    conv = _conv(prob, options=WP_OPTS)
    y0 = _run(conv, prob, "conv_pw_glds_256x256p")
    conv.set_option("pw256wp_stagger", stagger)
    y = _run(conv, prob, "conv_pw_glds_256x256p")
    _hold(y, prob, FP32_TOL, f"pw256wp_stagger={stagger}")
    assert _same_bits(y, y0)


# ---- res_prefetch ----
@pytest.mark.parametrize("family,case,precision,options", [
    ("conv_pw_glds_128x64", (1, 21, 19, 160, 640), "fp32", {}),
    ("conv_pw_glds_128x128", (1, 21, 19, 160, 640), "fp32", {"pw64_maxtiles": 0}),
    ("conv_igemm_128x128x32", (1, 21, 19, 160, 640), "fp32", {"pw_glds": 0}),
    ("gemm_rs6_64x64", (1, 21, 19, 64, 640), "bf16x6", {}),
], ids=lambda c: c if isinstance(c, str) else ("x".join(map(str, c)) if isinstance(c, tuple) else "opts"))
def test_res_prefetch_0_with_a_residual_and_ragged_rows(problems, family, case, precision, options):
    """res_prefetch = 0: the epilogue loads every residual row inside its row loop instead of requesting a thread's first eight rows
    early (conv_res_prefetch).  The prefetch applies to whole tiles only, so K is short here (at most five k-tiles: no split) and M =
    399 leaves the last m-tile ragged -- the rows past the end are the ones the prefetch must not read.  Either way a value is
    acc * scale + shift, then + residual, then ReLU, in that order: bit for bit equal (the option moves a load, not an operation)."""
    prob = problems(*case)
    conv = _conv(prob, precision=precision, options=options)
    y1 = _run(conv, prob, family)
    conv.set_option("res_prefetch", 0)
    y0 = _run(conv, prob, family)
    tol = FP32_TOL if precision == "fp32" else RS_TOL[precision]
    _hold(y0, prob, tol, f"res_prefetch=0 {family}")
    _hold(y1, prob, tol, f"res_prefetch=1 {family}")
    assert _same_bits(y0, y1), f"{(y0 != y1).sum().item()} values differ"


# ---- split_model ----
def test_split_model_0_plans_the_tail_by_slots(problems):
    """plan_tail_split (conv_common.h) under split_model = 0 counts resident workgroup slots (two per CU for the 128 x 128 kernel)
    where the default counts CUs.  90 tiles of 16 k-tiles: cut three or four ways they are 270 / 360 workgroups -- one round of 512
    slots, so the slot model takes the four-way cut, but two workgroups on some of the 256 CUs, so the CU model stays with two.
    Another cut of K is another order of the sum: the two results must DIFFER in some bit (that is what shows the other plan was
    made -- and that both launches went through the split-K reduce, which adds the residual), both hold the reference, and
    they lie within the operator tolerance of each other."""
    prob = problems(2, 25, 25, 512, 1152)
    conv = _conv(prob)
    y1 = _run(conv, prob, "conv_pw_glds_128x128")
    conv.set_option("split_model", 0)
    y0 = _run(conv, prob, "conv_pw_glds_128x128")
    _hold(y0, prob, FP32_TOL, "split_model=0")
    _hold(y1, prob, FP32_TOL, "split_model=1")
    assert not _same_bits(y0, y1), "the slot model made the CU model's plan: the option had no effect at this shape"
    _mutual(y0, y1, prob, FP32_TOL, "split_model 0 / 1")


# ---- gates ----
def test_pw256_mintiles_brings_a_small_layer_onto_the_256x128_kernel(problems):
    """K = 1024 (the kernel's default channel gate) and M x cout = 399 x 256: four 256 x 128 tiles, far under the default 256.
    pw256_mintiles = 1 opens the gate (family asserted on both sides).  The tail plan depends on the tile count (four tiles against
    eight), so the cut of K -- the order of the sums -- may differ between the two kernels: they are held to the reference and to
    each other at the operator tolerance, with no claim to the bit.  (At this shape both plans cut K eight ways and the printed
    distance is 0.)"""
    prob = problems(1, 21, 19, 1024, 256)
    y1 = _run(_conv(prob), prob, "conv_pw_glds_128x128")
    y0 = _run(_conv(prob, options={"pw256_mintiles": 1}), prob, "conv_pw_glds_256x128")
    _hold(y0, prob, FP32_TOL, "pw256_mintiles=1 (conv_pw_glds_256x128)")
    _hold(y1, prob, FP32_TOL, "pw256_mintiles=256 (conv_pw_glds_128x128)")
    _mutual(y0, y1, prob, FP32_TOL, "256 x 128 against 128 x 128 tiles")


@pytest.mark.parametrize("case,fam16,fam32", [((1, 15, 13, 64, 96, 3, 1), "conv_igemm_128x64x16", "conv_igemm_128x64x32"),
                                             ((2, 15, 13, 320, 160, 3, 2), "conv_igemm_128x128x16", "conv_igemm_128x128x32"),
                                             ((1, 21, 19, 32, 32, 3, 1), "conv_igemm_128x32x16", "conv_igemm_128x32x32")],
                         ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else c)
def test_fp32_bk_16_forces_16_channel_k_tiles(problems, case, fam16, fam32):
    """fp32_bk = 16 (create-time: the weights are packed for the k-tile) on 3x3 layers whose channels are a multiple of 32 and which
    therefore run 32-channel k-tiles by default, in the three tile widths, with dilation 2 on one.  Twice as many k-tiles of half
    the width: another order of the sum (and another tail plan), so the two are held to the reference and to each other at the
    operator tolerance."""
    B, H, W, cin, cout, k, dil = case
    prob = problems(B, H, W, cin, cout, k=k, dil=dil)
    y32 = _run(_conv(prob, k=k, dil=dil, conv_algo="direct"), prob, fam32)
    y16 = _run(_conv(prob, k=k, dil=dil, conv_algo="direct", options={"fp32_bk": 16}), prob, fam16)
    assert fam16.endswith("x16")
    _hold(y16, prob, FP32_TOL, f"fp32_bk=16 {fam16}")
    _hold(y32, prob, FP32_TOL, f"fp32_bk=0 {fam32}")
    _mutual(y16, y32, prob, FP32_TOL, "16- against 32-channel k-tiles")


def test_fp32_bk_is_refused_on_a_live_handle(problems):
    from peanut_amd import _lib
    prob = problems(1, 15, 13, 64, 96, k=3)
    conv = _conv(prob, k=3, conv_algo="direct")
    for key in ("fp32_bk", "rs_conv", "rs_bn64_maxk"):
        with pytest.raises(_lib.PeanutHipError):
            conv.set_option(key, 0)
    _run(conv, prob, "conv_igemm_128x64x32")


@pytest.mark.parametrize("precision", ["bf16x6", "bf16x3", "fp16x3"])
@pytest.mark.parametrize("case,algo,family", [((1, 15, 13, 64, 96, 3, 1), "auto", "conv_igemm_128x64x32"),
                                             ((1, 15, 13, 128, 128, 3, 2), "direct", "conv_igemm_128x64x32"),
                                             ((1, 9, 11, 320, 160, 3, 1), "direct", "conv_igemm_128x128x32")],
                         ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else c)
def test_rs_conv_0_keeps_3x3_convs_on_the_fp32_kernel(problems, case, algo, family, precision):
    """rs_conv = 0 (create-time) in every emulated mode: a 3x3 conv is not packed for conv_rs.hip, reports PEANUT_PREC_FP32
    through peanut_conv_precision, runs conv_igemm and equals the fp32 handle bit for bit (same packed weights, same kernel, same
    launch) -- while the same layer with the default rs_conv = 1 reports the mode and runs conv_rs.  Held to the reference at the
    fp32 kernels' tolerance."""
    from peanut_amd import _lib
    B, H, W, cin, cout, k, dil = case
    prob = problems(B, H, W, cin, cout, k=k, dil=dil)
    lib = _lib.load()
    fp32 = _conv(prob, k=k, dil=dil, conv_algo=algo)
    off = _conv(prob, k=k, dil=dil, conv_algo=algo, precision=precision, options={"rs_conv": 0})
    on = _conv(prob, k=k, dil=dil, conv_algo=algo, precision=precision)
    assert lib.peanut_conv_precision(off._h) == _lib.PRECISIONS["fp32"]
    assert lib.peanut_conv_precision(on._h) == _lib.PRECISIONS[precision]
    y = _run(off, prob, family)
    _hold(y, prob, FP32_TOL, f"{precision} rs_conv=0 {family}")
    assert _same_bits(y, _run(fp32, prob, family))
    y_on = _run(on, prob, "conv_" + RS_TAG[precision] + "128x" + ("128" if cout >= 128 else "64"))
    _hold(y_on, prob, RS_TOL[precision], f"{precision} rs_conv=1")


# ---- gemm_rs tile gates: rs64_maxk / rs64_maxtiles, rs256_mink / rs256_mintiles, rs_bn64_maxk ----
RS_GATE_CASES = [
    # (B, H, W, cin, cout), options, family without the piece count, input channels of the first source (None: one source)
    ((1, 21, 19, 160, 512), {}, "64x64", None),                                                    # default: few tiles, short K
    ((1, 21, 19, 160, 512), {"rs64_maxtiles": 0}, "128x128", None),                                # tile gate closed
    ((1, 21, 19, 160, 512), {"rs64_maxk": 128}, "128x128", None),                                  # channel gate below this K
    ((1, 21, 19, 1024, 256), {"rs64_maxk": 1024}, "64x64", None),                                  # channel gate raised to a K = 1024 layer (128x128 by default, RS_CASES)
    ((3, 75, 75, 256, 128), {"rs64_maxtiles": 1024}, "64x64", None),                               # tile gate raised: 132 tiles of 128 rows (128x128 by default, RS_CASES)
    ((1, 21, 19, 64, 256), {"rs64_maxtiles": 0}, "128x64", None),                                  # 64-wide packed (K <= rs_bn64_maxk = 128)
    ((1, 21, 19, 256, 256), {"rs64_maxtiles": 0, "rs_bn64_maxk": 256}, "128x64", None),            # rs_bn64_maxk raised: K = 256 packed 64 wide
    ((1, 21, 19, 64, 256), {"rs64_maxtiles": 0, "rs_bn64_maxk": 0}, "128x128", None),              # rs_bn64_maxk = 0: K = 64 packed 128 wide
    ((1, 21, 19, 64, 256), {"rs_bn64_maxk": 0}, "64x64", None),                                    # ... and the 64 x 64 kernel on halves of those tiles
    ((1, 21, 19, 160, 512), RS256_OPTS, "256x256", None),                                          # 2 x 2 tiles, the last 256-row tile ragged (M = 399)
    ((1, 21, 19, 160, 512), {**RS256_OPTS, "rs64_maxtiles": 128, "rs64_maxk": 128}, "256x256", None),   # ... reached past the other 64 x 64 gate
    ((1, 21, 19, 160, 512), RS256_OPTS, "256x256", 64),                                            # two sources: 64 + 96 channels, switch after k-tile 4
    ((1, 21, 19, 160, 512), {"rs256_mink": 64, "rs256_mintiles": 4, "rs64_maxtiles": 0}, "128x128", None),   # 399 x 512 outputs: under four 256 x 256 tiles
    ((1, 21, 19, 160, 512), {"rs256_mink": 192, "rs256_mintiles": 1, "rs64_maxtiles": 0}, "128x128", None),  # K = 160 under the channel gate
]


@pytest.mark.parametrize("precision", ["bf16x6", "bf16x3", "fp16x3"])
@pytest.mark.parametrize("case,options,family,c1", RS_GATE_CASES,
                         ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else (c if isinstance(c, str) else ("opts" if isinstance(c, dict) else f"c1_{c}")))
def test_register_split_gemm_tile_gates(problems, case, options, family, c1, precision):
    """Each gate of gemm_rs.hip moved so that a layer of a few tiles lands on each of its four kernels -- 64 x 64, 128 x 64, 128 x 128,
    256 x 256 -- in every emulated mode, family asserted per mode; rs_bn64_maxk (create-time) changes the packing the kernels read.
    The gated-in 256 x 256 kernel runs a ragged last tile, a two-source layer and split-K parts on 2 x 2 tiles (its smallest case so
    far was 8 x 64 x 64 x 512 x 512).  Other tiles cut K differently, so there is no bit-for-bit claim between gates: every case is
    held to the reference at the mode's tolerance, with a residual and ReLU."""
    prob = problems(*case)
    conv = _conv(prob, precision=precision, options=options)
    y = _run(conv, prob, "gemm_" + RS_TAG[precision] + family, c1=c1)
    _hold(y, prob, RS_TOL[precision], f"{precision} {family} {case} {options} c1={c1}")


@pytest.mark.parametrize("key,value,start,before,after", [
    ("rs256_mink", 64, {"rs256_mintiles": 1, "rs64_maxtiles": 0}, "gemm_rs6_128x128", "gemm_rs6_256x256"),
    ("rs256_mintiles", 1, {"rs256_mink": 64, "rs64_maxtiles": 0}, "gemm_rs6_128x128", "gemm_rs6_256x256"),
    ("rs64_maxk", 128, {}, "gemm_rs6_64x64", "gemm_rs6_128x128"),
    ("rs64_maxtiles", 0, {}, "gemm_rs6_64x64", "gemm_rs6_128x128"),
], ids=lambda c: c if isinstance(c, str) else ("opts" if isinstance(c, dict) else str(c)))
def test_rs_gates_are_run_time_options(problems, key, value, start, before, after):
    """The four gemm_rs gates are read at every launch: set_option on a live handle moves the layer to another kernel (rs_bn64_maxk,
    which shapes the packed weights, is refused there: test_fp32_bk_is_refused_on_a_live_handle)."""
    prob = problems(1, 21, 19, 160, 512)
    conv = _conv(prob, precision="bf16x6", options=start)
    _run(conv, prob, before)
    conv.set_option(key, value)
    y = _run(conv, prob, after)
    _hold(y, prob, RS_TOL["bf16x6"], f"{key}={value} -> {after}")
