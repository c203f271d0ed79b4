"""Test helpers the GPU tests of the image passes share (tests/test_gpu_denoise.py, test_gpu_variance.py, test_gpu_reproject.py):
the sizes and pass counts every filter path is run at, a camera pose, pixel lists, bit views, host arrays wrapped as textures, and
the error check."""
import numpy as np
import pytest

from tdt4230_project_raytracing_amd import rt

INSIDE_TURNED = ((0.1, 0.05, -0.6), 135.0, 10.0, 70.0)                          # (origin, yaw, pitch, fov) inside config1's room
# narrower than the 5x5 and 7x7 windows, one tile, a ragged edge in each direction, wider and taller than any tile
SIZES = [(1, 1), (2, 2), (5, 5), (33, 17), (64, 48), (257, 19), (19, 257)]
PASSES = [1, 2, 3, 5, 8]                                                        # both scratch sequences, LDS tiles and gathers


def _all_pixels(w, h):
    return np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)     # row-major: y outer, x inner


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _wrapped(ctx, a):
    """A host array as a torch tensor on the GPU, wrapped (not bound) as a texture of its height and width."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(a.shape[0], a.shape[1], 4).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, rt.Texture.wrap_device(ctx, t.data_ptr(), a.shape[1], a.shape[0], bind=False)


def _raises(code, fn, *args, **kw):
    with pytest.raises(rt.TdtError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
