"""Procedural frames of the video-output goldens (tests/golden/video_output_*.npz, scripts/make_golden_video_output.py):
pixel (frame f, channel c, row y, column x) = an integer hash of (seed, f, c, y, x) in 0..255, times 2^-8, so every value
is exact in float32 wherever it is computed.  The same expression runs on numpy int64 arrays (the CPU tests evaluate it
at the observed pixels only) and on torch int64 tensors (the GPU tests build whole frames on the device)."""
import numpy as np
import torch

_M32 = 0xFFFFFFFF


def pixel_hash(seed, f, c, y, x):
    """int64 arrays / tensors (broadcast; f, c, y, x < 2^16) -> the hash in 0..255 (int64).  Every product stays below
    2^63: inputs below 2^32 times constants below 2^31."""
    h = (seed * 0x165667B1 + f * 0x2545F491 + c * 0x1B873593 + y * 0x5BD1E995 + x * 0x27D4EB2F) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & _M32
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & _M32
    h = h ^ (h >> 15)
    return h & 255


def pixel_values(seed, f, y, x):
    """numpy: float32 (n, 3) colours of the pixels (f[i], :, y[i], x[i]) (indices already wrapped into the frame)."""
    f, y, x = (np.asarray(a, np.int64)[:, None] for a in (f, y, x))
    c = np.arange(3, dtype=np.int64)[None]
    return (pixel_hash(int(seed), f, c, y, x).astype(np.float32) * np.float32(2.0 ** -8)).astype(np.float32)


def frames_numpy(seed, f0, f1, H, W):
    """(f1 - f0, 3, H, W) float32 frames on the host."""
    f = np.arange(f0, f1, dtype=np.int64)[:, None, None, None]
    c = np.arange(3, dtype=np.int64)[None, :, None, None]
    y = np.arange(H, dtype=np.int64)[None, None, :, None]
    x = np.arange(W, dtype=np.int64)[None, None, None, :]
    return (pixel_hash(int(seed), f, c, y, x).astype(np.float32) * np.float32(2.0 ** -8)).astype(np.float32)


def frames_torch(seed, f0, f1, H, W, device, out=None):
    """(f1 - f0, 3, H, W) float32 frames built on `device` (into `out` when given), one frame at a time."""
    if out is None:
        out = torch.empty((f1 - f0, 3, H, W), dtype=torch.float32, device=device)
    c = torch.arange(3, dtype=torch.int64, device=device)[:, None, None]
    y = torch.arange(H, dtype=torch.int64, device=device)[None, :, None]
    x = torch.arange(W, dtype=torch.int64, device=device)[None, None, :]
    for k, f in enumerate(range(f0, f1)):
        out[k] = pixel_hash(int(seed), f, c, y, x).to(torch.float32) * (2.0 ** -8)
    return out
