"""The reference's visualisation frame (``Agent_Helper._visualize``, nav/agent/agent_helper.py:496-621, with ``init_vis_image`` and
``get_contour_points`` of nav/agent/utils/visualization.py) rendered on the device (csrc/vis.hip): the uint8 ``[600, 1415, 3]`` BGR
``vis_image`` from the maps where they lie, three launches for 1..16 episodes, instead of C + 2 plane downloads, a PIL palette
pass, three matplotlib colour-map passes, three ``cv2.resize`` calls and a scikit-image dilation per step on the host.

Pinned bit for bit by the reference's own code (tools/gen_golden_vis.py -> tests/golden/vis_golden.npz): the index map, the whole
frame without the arrow, the arrow's vertices and colour, the file name.  UNPINNED, because cv2 is absent where the fixtures are
made: the arrow's fill (a pixel is painted iff its integer centre lies in the closed polygon), the nearest resize at map sizes
that do not divide 480 (stated rule: cv2's legacy ``INTER_NEAREST``), the four titles (drawn only where ``cv2`` imports) and the
JPEG bytes (PIL writes the file).

Nothing here imports matplotlib: the ``Purples`` table is committed below (tools/gen_golden_vis.py regenerates it, a CPU test
re-derives it where matplotlib imports).  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib

H, W = _lib.VIS_H, _lib.VIS_W

# int(x * 255.) of the 24 colours of the reference's palette (nav/constants.py: color_palette; agent_helper.py:545), RGB
_PALETTE_RGB = (
    255, 255, 255, 153, 153, 153, 229, 229, 229, 244, 91, 66, 31, 120, 180, 239, 199, 168, 239, 226, 168, 226, 239, 168,
    199, 239, 168, 172, 239, 168, 168, 239, 190, 168, 239, 217, 168, 235, 239, 168, 208, 239, 168, 181, 239, 181, 168, 239,
    208, 168, 239, 235, 168, 239, 239, 168, 217, 239, 168, 190, 76, 168, 217, 239, 15, 217, 239, 168, 141, 86, 244, 64)


def palette_lut() -> np.ndarray:
    """uint8 [256, 3] RGB: what ``putpalette(color_pal)`` / ``convert("RGB")`` give for every index (zero beyond the palette)."""
    lut = np.zeros(768, np.uint8)
    lut[:len(_PALETTE_RGB)] = _PALETTE_RGB
    return lut.reshape(256, 3)


# (cm(i)[[2, 1, 0]] * 255).astype(uint8) of matplotlib's 'Purples' for i = 0..255, then the "bad" colour (NaN): 257 BGR triples.
# NOT k / 255 * 255 recomputed: several entries truncate one below what they round to.
_PURPLES_BGR_HEX = (
    "fdfbfcfcfafbfcfafbfcf9fafbf9fafbf8f9fbf8f9fbf7f9faf7f8faf7f8faf6f7faf6f7f9f5f7f9f5f6f9f4f6f9f4f5f8f3f5f8f3f5f8f3f4f8f2f4f7f2f3"
    "f7f1f3f7f1f3f7f0f2f6f0f2f6f0f1f6eff1f6eff0f5eef0f5eef0f5edeff5edeff4eceef4eceef4ebedf4ebecf3eaecf3e9ebf3e9eaf2e8eaf2e8e9f2e7e8"
    "f1e6e8f1e6e7f1e5e7f0e5e6f0e4e5f0e3e5efe3e4efe2e3efe2e3efe1e2eee1e1eee0e1eedfe0eddfdfeddedfeddedeecddddecdcddecdcdcebdbdbebdbdb"
    "ebdadaead9d9ead8d8e9d7d7e9d7d6e9d6d6e8d5d5e8d4d4e7d3d3e7d2d2e6d1d1e6d0d0e5cfcfe5cecee4cdcde4cdcce3cccbe3cbcae2cac9e2c9c8e1c8c7"
    "e1c7c6e1c6c6e0c5c5e0c4c4dfc3c3dfc3c2dec2c1dec1c0ddc0bfddbfbedcbebddcbdbcdbbcbbdbbbbadabab9d9b9b8d9b8b7d8b7b6d8b6b6d7b4b5d6b3b4"
    "d6b2b3d5b1b2d4b0b1d4afb0d3aeafd2adaed2acadd1abacd1a9abd0a8aacfa7a9cfa6a8cea5a7cda4a6cda3a6cca2a5cca1a4cba0a3ca9ea2ca9da1c99ca0"
    "c89b9fc89a9ec7999dc7989cc6979bc6969ac69599c59498c59497c49396c49296c39195c39094c28f93c28e92c28d91c18c90c18b8fc08a8ec08a8dbf898c"
    "bf888bbe878abe8689be8588bd8487bd8386bc8286bc8185bb8084bb8083bb7f82ba7e81ba7d80b97c7fb87a7eb8797eb7777db6767cb5757cb5737bb4727a"
    "b3717ab36f79b26e78b16c77b06b77b06a76af6875ae6775ae6674ad6473ac6373ab6172ab6071aa5f71a95d70a85c6fa85b6fa7596ea6586da6566ca5556c"
    "a4546ba3526aa3516aa25069a14e68a14d68a04c67a04a669f49669e48659e46649d45639c44639c42629b41619b40619a3e60993d5f993c5f983a5e97395d"
    "97385d96365c95355b95345a94335a943159933058922f58922d57912c56902b569029558f28548f27548e25538d24528d23528c22518c21508b1f508b1e4f"
    "8a1d4e891c4e891a4d88194c88184c87174b87164a86144a861349851248841148840f47830e46830d46820c45820b448109448008438007427f06427f0441"
    "7e03407e02407d013f7d003f000000")


def purples_bgr() -> np.ndarray:
    """uint8 [257, 3] BGR: entry i < 256 the colour of ``int(normed * 256)`` = i, entry 256 the colour of NaN (black)."""
    return np.frombuffer(bytes.fromhex(_PURPLES_BGR_HEX), np.uint8).reshape(257, 3).copy()


def arrow_colour() -> tuple:
    """``(int(p[11] * 255), int(p[10] * 255), int(p[9] * 255))`` (:605-607): the BGR colour of the agent's arrow."""
    return tuple(int(v) for v in _PALETTE_RGB[11:8:-1])


def arrow_pos(pose_pred, m: int, map_resolution) -> tuple:
    """``pos`` of :595-601 from the seven planner pose inputs, in the caller's float64."""
    start_x, start_y, start_o, gx1, gx2, gy1, gy2 = pose_pred
    gx1, gy1 = int(gx1), int(gy1)
    return ((start_x * 100. / map_resolution - gy1) * 480 / m,
            (m - start_y * 100. / map_resolution + gx1) * 480 / m,
            np.deg2rad(-start_o))


def contour_points(pos, origin=(670, 50), size=12) -> np.ndarray:
    """``get_contour_points`` (utils/visualization.py:5-16): the arrow's four vertices, int [4, 2] as (x, y) frame pixels.  On the
    host in float64: ``np.cos`` / ``np.sin`` own the last bit, the device gets integers."""
    x, y, o = pos
    pts = [(int(x) + origin[0], int(y) + origin[1])]
    for r, a in ((size / 1.5, o + np.pi * 4 / 3), (size, o), (size / 1.5, o - np.pi * 4 / 3)):
        pts.append((int(x + r * np.cos(a)) + origin[0], int(y + r * np.sin(a)) + origin[1]))
    return np.array(pts)


def init_vis_image(goal_name, legend) -> np.ndarray:
    """``init_vis_image`` (utils/visualization.py:27-83): white, the grey outlines, the legend; the four titles only where ``cv2``
    imports (unpinned)."""
    img = np.full((H, W, 3), 255, np.uint8)
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        font, colour = cv2.FONT_HERSHEY_DUPLEX, (20, 20, 20)
        for text, x0, width, y0 in (("RGB Observation (Target: {})".format(goal_name), 15, 640, 0),
                                    ("Semantic Map & Prediction", 640 + 30, 480, 0),
                                    ("Dist Weight", 640 + 480 + 45, 240, 0), ("Value Map", 640 + 480 + 45, 240, 530)):
            size = cv2.getTextSize(text, font, 1, 1)[0]
            img = cv2.putText(img, text, ((width - size[0]) // 2 + x0, y0 + (50 + size[1]) // 2), font, 1, colour, 1, cv2.LINE_AA)
    grey = [100, 100, 100]                                             # :66-77
    img[49, 15:655] = grey
    img[49, 670:1150] = grey
    for c in (14, 655, 669, 1150, 1164):
        img[50:530, c] = grey
    img[530, 15:655] = grey
    img[530, 670:1150] = grey
    if legend is not None:                                             # :80-81
        lx, ly = legend.shape[:2]
        img[537:537 + lx, 582 - ly // 2:582 - ly // 2 + ly, :] = legend
    return img


def load_legend(legend):
    """An array (taken as BGR, as ``cv2.imread`` gives it) or a path read with PIL; cropped ``[:118]`` (agent_helper.py:102)."""
    if legend is None:
        return None
    if isinstance(legend, (str, os.PathLike)):
        from PIL import Image
        legend = np.asarray(Image.open(legend).convert("RGB"))[:, :, ::-1]
    legend = np.ascontiguousarray(np.asarray(legend, np.uint8)[:118])
    if legend.ndim != 3 or legend.shape[2] != 3 or legend.shape[0] + 537 > H or legend.shape[1] > 2 * 582:
        raise ValueError(f"the legend must be [<= 63 after the crop, <= 1164, 3], got {legend.shape}")
    return legend


def resolve_stg(stg, m: int):
    """``int(stg[0])``, ``int(stg[1])`` (:520-521), checked: a coordinate below ``-m`` is NumPy's IndexError in the reference."""
    if stg is None:
        return m, m                                                    # no short-term goal yet: nothing is marked
    r, c = int(stg[0]), int(stg[1])
    if r < m and c < m and (r < -m or c < -m):
        raise ValueError(f"stg {(r, c)} indexes outside the {m} x {m} map")
    return r, c


_FIELD_BITS = {torch.float32: 32, torch.float64: 64}


class VisRenderer:
    """``render(**item)`` / ``render_batch(items)`` -> uint8 HIP tensor ``[600, 1415, 3]`` / ``[E, 600, 1415, 3]`` (BGR, the
    reference's ``vis_image``); the tensor is this object's buffer and is overwritten by the next call.  ``frame_host()`` reads the
    last result back into one pinned buffer and returns that buffer (valid until the next ``frame_host``).

    An item (all maps HIP tensors, read where they lie):
      local_map [4 + ncat, m, m] fp32 (unit column stride; a view into the full map is fine), collision_map / visited_vis uint8
      [full_w, full_h], lmb (gx1, gx2, gy1, gy2), goal uint8 [m, m], stg (the planner's ``self.stg``, or None), pose_pred (the
      seven planner pose inputs), goal_name; optional rgb uint8 [480, 640, 3] RGB, target_pred / value / dd_wt [m, m] with
      target_bits 32 | 64 (the arithmetic the reference normalises target_pred in: 64 when its prediction window is smaller than
      the full map, :362); ``arrow`` int [4, 2] replaces the vertices formed from pose_pred (tests)."""

    def __init__(self, args, device, legend=None):
        self.args = args
        self.device = torch.device(device)
        self.legend = load_legend(legend)
        self.ncat = int(args.num_sem_categories)
        self._palette = torch.from_numpy(palette_lut()).to(self.device)
        self._cmap = torch.from_numpy(purples_bgr()).to(self.device)
        self._backgrounds = {}
        self._frames = None
        self._index = None
        self._ranges = None
        self._host = None
        self._n_last = 0

    def background(self, goal_name) -> torch.Tensor:
        bg = self._backgrounds.get(goal_name)
        if bg is None:
            bg = torch.from_numpy(init_vis_image(goal_name, self.legend)).to(self.device)
            self._backgrounds[goal_name] = bg
        return bg

    def _buffers(self, E, m):
        if self._frames is None:
            self._frames = torch.empty((_lib.VIS_MAX_BATCH, H, W, 3), dtype=torch.uint8, device=self.device)
            self._ranges = torch.empty((_lib.VIS_MAX_BATCH, _lib.VIS_RANGE_WORDS), dtype=torch.int64, device=self.device)
        if self._index is None or self._index.shape[1] != m:
            self._index = torch.empty((_lib.VIS_MAX_BATCH, m, m), dtype=torch.uint8, device=self.device)

    def _episode(self, e, item, m, full):
        lm = item["local_map"]
        if not isinstance(lm, torch.Tensor) or not lm.is_cuda or lm.dtype != torch.float32 or lm.dim() != 3 or \
                tuple(lm.shape) != (4 + self.ncat, m, m) or lm.stride(2) != 1:
            raise ValueError(f"episode {e}: local_map must be an fp32 HIP tensor [{4 + self.ncat}, {m}, {m}] with unit column stride")
        ep = _lib.VisEpisodeC(local_map=lm.data_ptr(), plane_stride=int(lm.stride(0)), row_stride=int(lm.stride(1)))
        keep = [lm]
        for name in ("collision_map", "visited_vis"):
            t = item[name]
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or tuple(t.shape) != full or not t.is_contiguous():
                raise ValueError(f"episode {e}: {name} must be a contiguous uint8 HIP tensor {full}")
            setattr(ep, name, t.data_ptr())
        goal = item["goal"]
        if not isinstance(goal, torch.Tensor):                         # the host form of planner_inputs: float64 0 / 1
            goal = torch.as_tensor(np.ascontiguousarray(np.asarray(goal) != 0).astype(np.uint8)).to(self.device)
        if goal.dtype != torch.uint8 or tuple(goal.shape) != (m, m) or not goal.is_contiguous() or not goal.is_cuda:
            raise ValueError(f"episode {e}: goal must be a contiguous uint8 [{m}, {m}] HIP tensor")
        ep.goal = goal.data_ptr()
        keep.append(goal)
        ep.lmb[:] = [int(v) for v in item["lmb"]]
        ep.stg[:] = resolve_stg(item.get("stg"), m)
        rgb = item.get("rgb")
        if rgb is not None:
            if not isinstance(rgb, torch.Tensor):
                rgb = torch.as_tensor(np.ascontiguousarray(rgb)).to(self.device)
            if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (480, 640, 3):
                raise ValueError(f"episode {e}: rgb must be uint8 [480, 640, 3], got {rgb.dtype} {tuple(rgb.shape)}")
            rgb = rgb.contiguous()
            ep.rgb = rgb.data_ptr()
            keep.append(rgb)
        tp = item.get("target_pred")
        if tp is not None:
            fields = (tp, item.get("value"), item.get("dd_wt"))
            bits = (int(item.get("target_bits", 32)), 64, 64)
            for f, (name, t) in enumerate(zip(("target_pred", "value", "dd_wt"), fields)):
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in _FIELD_BITS or tuple(t.shape) != (m, m):
                    raise ValueError(f"episode {e}: {name} must be a float32 / float64 HIP tensor [{m}, {m}] (value and dd_wt come "
                                     "with target_pred: GeodesicSolver.fields())")
                t = t.contiguous()
                keep.append(t)
                ep.data_bits[f] = _FIELD_BITS[t.dtype]
                ep.bits[f] = max(bits[f], ep.data_bits[f]) if f else bits[f]
                if ep.bits[f] not in (32, 64) or ep.bits[f] < ep.data_bits[f]:
                    raise ValueError(f"episode {e}: target_bits {bits[f]} for a {t.dtype} target_pred")
            ep.target_pred, ep.value, ep.dd_wt = (t.data_ptr() for t in keep[-3:])
        if item.get("arrow") is not None:                              # (tests: vertices the pose arithmetic cannot produce)
            pts = np.asarray(item["arrow"], np.int64).reshape(4, 2)
        else:
            pts = contour_points(arrow_pos(item["pose_pred"], m, self.args.map_resolution))
        for k in range(4):
            ep.arrow[k][0], ep.arrow[k][1] = int(pts[k][0]), int(pts[k][1])
        ep.arrow_bgr[:] = (*arrow_colour(), 0)
        ep.index_map = self._index[e].data_ptr()
        ep.ranges = self._ranges[e].data_ptr()
        ep.frame = self._frames[e].data_ptr()
        return ep, keep

    def _common(self, m, full, goal_name):
        return _lib.VisCommonC(m=m, channels=4 + self.ncat, full_w=full[0], full_h=full[1], background=self.background(goal_name).data_ptr(),
                               palette=self._palette.data_ptr(), cmap=self._cmap.data_ptr(), stream=_lib.current_stream_ptr(self.device))

    def render_batch(self, items) -> torch.Tensor:
        """E <= 16 episodes of one map size and one goal name per call in three launches; frame e has the bits of ``render``.
        Episodes with different goal names (different title bars) are rendered in one call per name."""
        return self.launch(self.prepare(items))

    def prepare(self, items):
        """The host half of ``render_batch``: every check, the argument structs, the arrow's vertices -> what ``launch`` takes.  It
        holds the items' tensors and the addresses of this renderer's buffers; it is valid until the next ``prepare`` with another
        map size."""
        items = list(items)
        E = len(items)
        if E < 1 or E > _lib.VIS_MAX_BATCH:
            raise ValueError(f"render_batch takes 1..{_lib.VIS_MAX_BATCH} episodes, got {E}")
        m = int(items[0]["local_map"].shape[1])
        full = tuple(int(v) for v in items[0]["collision_map"].shape)
        self._buffers(E, m)
        built = [self._episode(e, it, m, full) for e, it in enumerate(items)]
        names = []
        for it in items:
            if it.get("goal_name", "") not in names:
                names.append(it.get("goal_name", ""))
        calls = []
        for name in names:
            which = [e for e, it in enumerate(items) if it.get("goal_name", "") == name]
            calls.append((name, (_lib.VisEpisodeC * len(which))(*[built[e][0] for e in which])))
        return dict(E=E, m=m, full=full, calls=calls, keep=[k for _, k in built])

    def launch(self, prepared) -> torch.Tensor:
        """The device half: one library call (three launches) per goal name on the current stream."""
        lib = _lib.load()
        with torch.cuda.device(self.device):
            for name, eps in prepared["calls"]:
                common = self._common(prepared["m"], prepared["full"], name)
                if len(eps) == 1:
                    rc, what = lib.peanut_vis_render(C.byref(common), C.byref(eps[0])), "peanut_vis_render"
                else:
                    rc, what = lib.peanut_vis_render_batch(C.byref(common), len(eps), eps), "peanut_vis_render_batch"
                _lib.check(rc, what)
        self._n_last = prepared["E"]
        return self._frames[:prepared["E"]]

    def render(self, **item) -> torch.Tensor:
        return self.render_batch([item])[0]

    def index_map(self, **item) -> torch.Tensor:
        """The index map alone (``peanut_vis_index_map``, one launch) -> uint8 HIP tensor [m, m] (this object's buffer)."""
        m = int(item["local_map"].shape[1])
        full = tuple(int(v) for v in item["collision_map"].shape)
        self._buffers(1, m)
        item = dict(item, target_pred=None, rgb=None)
        ep, keep = self._episode(0, item, m, full)
        with torch.cuda.device(self.device):
            common = self._common(m, full, item.get("goal_name", ""))
            _lib.check(_lib.load().peanut_vis_index_map(C.byref(common), C.byref(ep)), "peanut_vis_index_map")
        return self._index[0]

    def frame_host(self) -> np.ndarray:
        """The frames of the last call on the host, uint8 [E, 600, 1415, 3]: one pinned, stream-ordered read-back and no further
        copy -- the array IS the pinned buffer (as many frames as the largest batch so far) and is valid until the next
        ``frame_host``; copy what must outlive it."""
        if not self._n_last:
            raise RuntimeError("frame_host: nothing has been rendered")
        E = self._n_last
        if self._host is None or self._host.shape[0] < E:
            self._host = torch.empty((E, H, W, 3), dtype=torch.uint8).pin_memory()
        with torch.cuda.device(self.device):
            self._host[:E].copy_(self._frames[:E], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        return self._host[:E].numpy()


def sem_argmax(local_map: torch.Tensor) -> torch.Tensor:
    """``vlm = local_map[4:].clone(); vlm[-1] = 1e-5; vlm.argmax(0)`` (agent_state.py:259-262) in one launch -> uint8 HIP [m, m]."""
    lm = local_map
    if not lm.is_cuda or lm.dtype != torch.float32 or lm.dim() != 3 or lm.shape[1] != lm.shape[2] or lm.stride(2) != 1:
        raise ValueError(f"sem_argmax: a square fp32 [C, m, m] HIP tensor with unit column stride, got {tuple(lm.shape)} {lm.dtype}")
    out = torch.empty((lm.shape[1], lm.shape[2]), dtype=torch.uint8, device=lm.device)
    with torch.cuda.device(lm.device):
        common = _lib.VisCommonC(m=int(lm.shape[1]), channels=int(lm.shape[0]), stream=_lib.current_stream_ptr(lm.device))
        rc = _lib.load().peanut_vis_sem_argmax(C.byref(common), lm.data_ptr(), int(lm.stride(0)), int(lm.stride(1)), out.data_ptr())
    _lib.check(rc, "peanut_vis_sem_argmax")
    return out


def frame_path(args, rank, episode_no, timestep):
    """The reference's file name scheme (:500-505, :617-619) -> (episode directory, file name)."""
    dump_dir = "{}/dump/{}/".format(args.dump_location, args.exp_name)
    ep_dir = '{}/episodes/thread_{}/eps_{}/'.format(dump_dir, rank, episode_no - 1)
    fn = '{}/episodes/thread_{}/eps_{}/{}-{}-Vis-{}.jpg'.format(dump_dir, rank, episode_no - 1, rank, episode_no - 1, timestep)
    return ep_dir, fn


def write_frame(fn, frame_bgr: np.ndarray) -> None:
    """``cv2.imwrite(fn, vis_image, [cv2.IMWRITE_JPEG_QUALITY, 100])`` (:621) with PIL (the JPEG bytes are unpinned)."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(fn, format="JPEG", quality=100)
