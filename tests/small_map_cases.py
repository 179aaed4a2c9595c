"""The smallest maps the prediction forward accepts (test infrastructure, importable without a GPU): shapes, inputs and the fp64
reference shared by tests/test_small_maps_cpu.py and tests/test_small_maps_gpu.py.

``peanut_pred_forward`` takes any map with H, W >= 16 (csrc/pred_api.hip: get_plan); the stride-8 backbone leaves a 2 x 2 ... 6 x 6
feature map (or a 2 x 90 strip) there: pyramid scales 3 and 6 exceed the map, dilations 2 and 4 exceed it, every GEMM has a single
ragged row tile.  The reference has no lower bound, so the oracle (oracle/pspnet_ref.py) serves every shape; it is run in float64
(state dict and input cast, the oracle itself unchanged) and memoised per (cfg, shape), so that every variant of the GPU file
reuses one CPU run."""
from typing import Dict, Tuple

import torch

# (B, H, W) -> layer4 (h, w) after the stride-8 backbone, and what the shape is for
SMALL_MAPS = [
    (1, 16, 16),      # 2 x 2: the smallest legal map; scales 3 and 6 DOWN-sample, dilation 2 / 4 leave empty sub-grids, M = 4
    (9, 16, 16),      # 2 x 2: the batch opens the row-per-wave pyramid-term gate and closes the skinny-GEMM gate (B * 36 > 64)
    (2, 17, 23),      # 3 x 3: odd at every stride-2 stage (17 -> 9 -> 5 -> 3, 23 -> 12 -> 6 -> 3)
    (1, 24, 56),      # 3 x 7: rectangular; six bins over 3 rows and over 7 columns
    (1, 16, 720),     # 2 x 90: strip
    (1, 720, 16),     # 90 x 2: strip, transposed
    (1, 31, 33),      # 4 x 5
    (1, 63, 16),      # 8 x 2
    (2, 47, 47),      # 6 x 6: scale 6 is the identity
    (1, 40, 41),      # 5 x 6
    (3, 23, 16),      # 3 x 2
]
LAYER4 = {
    (1, 16, 16): (2, 2), (9, 16, 16): (2, 2), (2, 17, 23): (3, 3), (1, 24, 56): (3, 7), (1, 16, 720): (2, 90),
    (1, 720, 16): (90, 2), (1, 31, 33): (4, 5), (1, 63, 16): (8, 2), (2, 47, 47): (6, 6), (1, 40, 41): (5, 6),
    (3, 23, 16): (3, 2),
}
CORE = SMALL_MAPS[:5]

TOL = 5e-5            # tests/test_pred_gpu.py: what the fp32 forward is held to on logits and on sigmoid outputs
MIN_SIDE = 16         # csrc/pred_api.hip, get_plan: H, W >= 16
BELOW_MIN = MIN_SIDE - 1

TAP_NAMES = ["stem0", "stem1", "stem2", "pool", "layer1", "layer2", "layer3", "layer4", "bottleneck", "logits_lowres"]


def shape_id(s) -> str:
    return "x".join(map(str, s))


def cfg_for(align_corners: bool = False):
    from peanut_amd.weights import PredCfg
    return PredCfg(align_corners=align_corners)


def inputs(shape: Tuple[int, int, int], channels: int = 14) -> torch.Tensor:
    """``tests/test_pred_gpu.py::_inputs`` with its seed h * 1000 + w."""
    b, h, w = shape
    g = torch.Generator().manual_seed(h * 1000 + w)
    return (torch.rand((b, channels, h, w), generator=g) > 0.7).float()


_SD: Dict[object, Dict[str, torch.Tensor]] = {}
_OUT: Dict[object, torch.Tensor] = {}
_TAPS: Dict[object, Dict[str, torch.Tensor]] = {}


def state_dict(cfg, dtype=torch.float32):
    """make_seeded_state_dict(cfg, 0), as it is (fp32: what the device gets) or cast to float64 (what the reference runs on)."""
    from peanut_amd.weights import make_seeded_state_dict
    key = (cfg, dtype)
    if key not in _SD:
        sd = make_seeded_state_dict(cfg, seed=0)
        _SD[key] = sd if dtype == torch.float32 else {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    return _SD[key]


def ref_logits(cfg, shape, dtype=torch.float64) -> torch.Tensor:
    """Logits of the oracle in ``dtype`` (float64: the reference; float32: the oracle as every other test uses it).  Shared,
    never written to."""
    from oracle import pspnet_ref
    key = (cfg, tuple(shape), dtype)
    if key not in _OUT:
        _OUT[key] = pspnet_ref.forward_batch(state_dict(cfg, dtype), inputs(shape, cfg.in_channels).to(dtype), cfg)
    return _OUT[key]


def ref_taps(cfg, shape, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    from oracle import pspnet_ref
    key = (cfg, tuple(shape), dtype)
    if key not in _TAPS:
        with torch.no_grad():
            _TAPS[key] = pspnet_ref.taps(state_dict(cfg, dtype), inputs(shape, cfg.in_channels).to(dtype), cfg)
    return _TAPS[key]
