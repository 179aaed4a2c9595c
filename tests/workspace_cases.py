"""Helpers of tests/test_workspace_gpu.py (test infrastructure, importable without a GPU): no result of the library may depend
on what its device memory held before the call.

``poisoned()``           library option ``debug_poison_alloc`` (csrc/options.h) for the handles created AND the calls made inside
                         the block: every device allocation the library makes for itself starts as 0xFF bytes (fp32 / fp64 NaN,
                         int -1, 64-bit keys all ones) instead of whatever the allocator returns -- on a fresh process, zeros.
``dirty_torch_cache()``  the same for the ``torch.empty`` outputs of the Python mirrors: blocks of the sizes about to be requested
                         are filled with 0xFF and handed back to torch's caching allocator, which serves the next request of that
                         size from them.
``same()``               bit equality over every field of a result.
"""
import numpy as np
import torch


def poisoned():
    """``with poisoned(): handle = ...; handle(...)`` -- wrap the creation and the calls: a handle snapshots the option when it is
    created, its arena is allocated on the first forward and grows later, and what a handle-less entry point allocates
    (peanut_map_reserve) follows the process default."""
    from peanut_amd import _lib
    return _lib.default_options(debug_poison_alloc=1)


def dirty_torch_cache(nbytes, device="cuda"):
    """Allocate, fill with 0xFF and free one torch block per entry of ``nbytes`` (an int or an iterable of ints)."""
    sizes = [nbytes] if isinstance(nbytes, int) else list(nbytes)
    blocks = [torch.full((max(int(n), 1),), 0xFF, dtype=torch.uint8, device=device) for n in sizes]
    torch.cuda.synchronize()
    del blocks


_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def same(a, b):
    """True when ``a`` and ``b`` hold the same bits in every field: tensors (``torch.equal`` on the bit patterns of floating-point
    tensors, so equal NaN positions count as equal and +0 / -0 as different), numpy arrays, dicts, lists / tuples, scalars."""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        a, b = torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
            return False
        if a.dtype != b.dtype or a.shape != b.shape or a.device.type != b.device.type:
            return False
        if a.dtype in _INT_VIEW:
            a, b = a.contiguous().view(_INT_VIEW[a.dtype]), b.contiguous().view(_INT_VIEW[b.dtype])
        return torch.equal(a, b)
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def first_difference(a, b, path="result"):
    """Where ``same`` fails, in words (for assertion messages)."""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        for k in a:
            if not same(a[k], b[k]):
                return first_difference(a[k], b[k], f"{path}[{k!r}]")
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            if not same(x, y):
                return first_difference(x, y, f"{path}[{i}]")
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype:
        x, y = a.detach().cpu(), b.detach().cpu()
        diff = (x != y) & ~((x != x) & (y != y)) if x.dtype.is_floating_point else (x != y)
        nan = int(((x != x) != (y != y)).sum()) if x.dtype.is_floating_point else 0
        return f"{path}: {int(diff.sum())} of {x.numel()} elements differ ({nan} of them NaN on one side only), shape {tuple(x.shape)}"
    return f"{path}: {a!r} against {b!r}"[:400]
