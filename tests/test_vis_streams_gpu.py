"""The stream contract of the visualisation renderer (include/peanut_hip.h: three launches on common->stream, "nothing
synchronises") with the protocols of tests/stream_cases.py, and its independence from what its workspaces held.  The entries take
their stream in a struct, like peanut_plan_mark, so they are held here and not in the prototype table of tests/test_streams_cpu.py.

* P1 on ``render`` (``peanut_vis_render``), ``render_batch`` (E = 3, ``peanut_vis_render_batch``), ``index_map``
  (``peanut_vis_index_map``) and ``sem_argmax`` (``peanut_vis_sem_argmax``): every input buffer is overwritten late behind a backlog
  and again right after the call; the result equals that of the idle default stream, and the call returns while the backlog is
  pending.
* One ``render_batch`` on a fresh renderer whose buffers (index maps, range words, frames) come from 0xFF-filled blocks, under the
  library's ``debug_poison_alloc``, equals a fresh renderer's plain result."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc
import vis_cases as vc
from peanut_amd import _lib
from peanut_amd import vis as pv
from workspace_cases import dirty_torch_cache, poisoned, same

pytestmark = pytest.mark.gpu

M, NCAT, FULL = 96, 10, 128
LMB = [16, 16 + M, 24, 24 + M]
ARGS = SimpleNamespace(num_sem_categories=NCAT, map_resolution=vc.RES)


def _inputs(E):
    """seed -> per episode (full_map, collision, visited, goal, rgb, target_pred, value, dd_wt) as CPU tensors, valid for every seed."""
    def build(seed):
        g = torch.Generator().manual_seed(613 * seed + 11)
        out = []
        for _ in range(E):
            full_map = torch.rand((4 + NCAT, FULL, FULL), generator=g) * 1.6
            full_map[4:, ::3] = 0.0
            out += [full_map, (torch.rand((FULL, FULL), generator=g) < 0.05).to(torch.uint8),
                    (torch.rand((FULL, FULL), generator=g) < 0.05).to(torch.uint8), (torch.rand((M, M), generator=g) < 0.002).to(torch.uint8),
                    (torch.rand((480, 640, 3), generator=g) * 256).to(torch.uint8), torch.rand((M, M), generator=g),
                    torch.rand((M, M), generator=g, dtype=torch.float64), torch.rand((M, M), generator=g, dtype=torch.float64)]
        return tuple(out)
    return build


def _items(x, E):
    items = []
    for e in range(E):
        fm, col, visd, goal, rgb, tp, value, dd = x[8 * e:8 * e + 8]
        items.append(dict(local_map=fm[:, LMB[0]:LMB[1], LMB[2]:LMB[3]], collision_map=col, visited_vis=visd, lmb=LMB, goal=goal,
                          stg=(7 + e, 90 - e), pose_pred=np.array([*vc.pose_at(M, (LMB[0], LMB[2]), 0.3 + 0.1 * e, 0.6, 40.0 * e), *LMB]),
                          goal_name="chair", rgb=rgb, target_pred=tp, value=value, dd_wt=dd, target_bits=64 if e % 2 else 32))
    return items


def _make():
    return pv.VisRenderer(ARGS, "cuda:0", legend=vc.legend())


def test_render_single_and_batched_behind_a_backlog():
    def single(r, x, outs):
        return r.render(**_items(x, 1)[0])
    sc.p1("peanut_vis_render", _make, single, sc.to_device(_inputs(1)(0)), sc.to_device(_inputs(1)(1)), "async")

    def batch(r, x, outs):
        return r.render_batch(_items(x, 3))
    sc.p1("peanut_vis_render_batch", _make, batch, sc.to_device(_inputs(3)(0)), sc.to_device(_inputs(3)(1)), "async")


def test_index_map_and_sem_argmax_behind_a_backlog():
    def index(r, x, outs):
        return r.index_map(**_items(x, 1)[0])
    sc.p1("peanut_vis_index_map", _make, index, sc.to_device(_inputs(1)(0)), sc.to_device(_inputs(1)(1)), "async")

    def argmax(r, x, outs):
        return pv.sem_argmax(x[0][:, LMB[0]:LMB[1], LMB[2]:LMB[3]])
    sc.p1("peanut_vis_sem_argmax", lambda: None, argmax, sc.to_device(_inputs(1)(0)), sc.to_device(_inputs(1)(1)), "async")


def test_render_batch_does_not_depend_on_what_its_buffers_held():
    x = sc.to_device(_inputs(3)(0))
    plain = _make().render_batch(_items(x, 3)).clone()
    torch.cuda.synchronize()
    with poisoned():
        dirty_torch_cache([_lib.VIS_MAX_BATCH * _lib.VIS_FRAME_BYTES, _lib.VIS_MAX_BATCH * _lib.VIS_RANGE_WORDS * 8, _lib.VIS_MAX_BATCH * M * M])
        r = _make()
        got = r.render_batch(_items(x, 3)).clone()
        torch.cuda.synchronize()
    assert same(got, plain)
    # and a second call on the used renderer, after another shape went through it
    small = next(c for c in vc.golden_cases() if c["name"] == "m8")
    r8 = dict(local_map=torch.from_numpy(small["full_map"]).cuda()[:, 8:16, 4:12], collision_map=torch.from_numpy(small["collision"]).cuda(),
              visited_vis=torch.from_numpy(small["visited"]).cuda(), lmb=small["lmb"], goal=torch.from_numpy(small["goal"]).cuda(), stg=None,
              pose_pred=np.array([*small["pose"], *small["lmb"]]), goal_name="chair")
    r.render(**r8)
    assert same(r.render_batch(_items(x, 3)).clone(), plain)
