#!/usr/bin/env python
"""What the two network planners decide and compute, as one JSON file, for whichever library is loaded (PEANUT_HIP_LIB or the
tree's): the op tables, the workspace bytes and SHA-256 digests of the outputs, at the smallest shapes that reach each branch
of the planners (csrc/pred_api.hip, csrc/rcnn_api.hip, csrc/net_common.h).  A refactor of the planners must leave the file
identical: run it once per library and diff.  Times are not recorded (they differ from run to run).

    python tools/plan_dump.py OUT.json
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]      # bench.synth_maps; the suite's small cases (tests/*_cases.py)

import torch  # noqa: E402

import bench  # noqa: E402
from peanut_amd import _lib  # noqa: E402
from peanut_amd.ops import FusedConv  # noqa: E402
from peanut_amd.prediction import HipSegmentor  # noqa: E402
from peanut_amd.rcnn import MaskRCNN  # noqa: E402
import rcnn_cases  # noqa: E402
import small_map_cases  # noqa: E402

DEV = "cuda:0"


def digest(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def pred_case(model: HipSegmentor, x: torch.Tensor, keep: bool = False) -> dict:
    b, _, h, w = x.shape
    model.debug_keep(keep)
    out = dict(logits=digest(model.forward_logits(x)), probs=digest(model.forward_logits(x, apply_sigmoid=True)))
    if keep:
        out["taps"] = {n: digest(model.debug_tensor(n)) for n in small_map_cases.TAP_NAMES}
    out["workspace_bytes"] = model.workspace_bytes(b, h, w)
    out["flops_per_map"] = model.flops_per_map(h, w)
    out["ops"] = [(name, kernel, flops, nbytes) for name, kernel, _ms, flops, nbytes in model.profile(x)]
    model.debug_keep(False)
    return out


def prediction() -> dict:
    cfg = small_map_cases.cfg_for()
    sd = small_map_cases.state_dict(cfg)
    maps = lambda b, s: bench.synth_maps(b, cfg.in_channels, s, DEV)  # noqa: E731
    side = small_map_cases.MIN_SIDE      # (bench.synth_maps needs a side above 16: this case takes the small-map suite's input)
    fp32 = HipSegmentor(cfg, sd, device=DEV)
    out = {f"fp32_1x{side}": pred_case(fp32, small_map_cases.inputs((1, side, side), cfg.in_channels).to(DEV)),
           "fp32_1x240": pred_case(fp32, maps(1, 240)),
           "fp32_2x480": pred_case(fp32, maps(2, 480)),
           "fp32_10x480": pred_case(fp32, maps(10, 480)),
           "fp32_1x240_keep": pred_case(fp32, maps(1, 240), keep=True)}
    del fp32
    out["bf16x6_2x480"] = pred_case(HipSegmentor(cfg, sd, device=DEV, precision="bf16x6"), maps(2, 480))
    return out


def detector() -> dict:
    cfg, sd, img = rcnn_cases.small_inputs()
    img = img.to(DEV)
    out = {}
    for overlap in (0, 1):
        for fused in (0, 1):
            with _lib.default_options(rcnn_fpn_overlap=overlap, rcnn_rpn_fused=fused):
                net = MaskRCNN(cfg, sd, device=DEV)
            for frames in (img[:1], img):
                b, h, w, _ = frames.shape
                pyr, obj, dl = net.forward_front(frames)
                det = net.inference(frames)
                out[f"overlap{overlap}_fused{fused}_b{b}"] = dict(
                    plan=net.plan(b, h, w),
                    front=[digest(t) for t in pyr + obj + dl],
                    detections=[{k: digest(v) for k, v in d.items()} for d in det],
                    ops=[(name, kernel, flops) for name, kernel, _ms, flops in net.probe_front(frames, reps=1)])
    return out


def fused_conv() -> dict:
    g = torch.Generator().manual_seed(0)
    conv = FusedConv(torch.randn((64, 64, 3, 3), generator=g) * 0.05, padding=1, relu=True, device=DEV,
                     options={"wino_min_cin": 64})       # (a single conv takes its Winograd form from 128 channels on by default)
    y = conv(torch.randn((1, 24, 24, 64), generator=g).to(DEV))
    return dict(kernel=_lib.load().peanut_last_conv_kernel().decode(), y=digest(y))


def main() -> None:
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    lib = _lib.load()
    doc = dict(abi=lib.peanut_abi_version(), prediction=prediction(), detector=detector(), fused_conv=fused_conv())
    with open(sys.argv[1], "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"plan_dump: wrote {sys.argv[1]} (library {_lib.lib_path()})")


if __name__ == "__main__":
    main()
