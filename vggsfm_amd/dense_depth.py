"""Dense depth alignment on the MI355X: the reference's ``dense_depth`` stage (vggsfm/runners/runner.py:744-814,
vggsfm/utils/utils.py:635-770) over ``vgg_sparse_depth`` / ``vgg_depth_align`` / ``vgg_depth_apply`` /
``vgg_depth_unproject`` (vggsfm_amd/csrc/dense.hip).

* :func:`sparse_depth` -- every observation of every 3D point projected into its image, grouped by image in the
  reference's order (images in order of first appearance in the point-major walk, observations in that walk's order).
* :func:`align` -- the per-image RANSAC fit ``disparity ~ scale * (1 / depth) + shift`` of scikit-learn 1.7's
  ``RANSACRegressor(LinearRegression(), min_samples=2, residual_threshold=median / 30, max_trials=20000)``, all images in
  one launch; ``samples`` replays recorded draws, otherwise they come from a generator on the device.
* :func:`apply` -- rescale, validate and invert the disparity maps in place (numpy float32 semantics, bit for bit).
* :func:`unproject` -- world points of the valid pixels (COLMAP's iterative undistortion per pixel).

Disparity maps are float32, as the depth model writes them.  There is no CPU path.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .reproj_video import _dev, _to_dev

ALIGN_STATUS = {0: "ok", 1: "no observation", 2: "ill-posed", 3: "no consensus set", 4: "fewer than 2 usable points",
                5: "recorded draws exhausted", 6: "recorded draw out of range"}
MAX_TRIALS = 20000

SparseDepth = namedtuple("SparseDepth", "names obs_ptr uvd xyzid")
Packed = namedtuple("Packed", "flat off heights widths max_pixels")
AlignResult = namedtuple("AlignResult", "scale shift n_trials n_inliers n_kept status kept inlier")


def _camera_rows(reconstruction, image_ids):
    """(S,3,4) [R|t] and (S,4) f, cx, cy, k (k = 0 for SIMPLE_PINHOLE) of the given images."""
    pose = np.zeros((len(image_ids), 3, 4))
    cam = np.zeros((len(image_ids), 4))
    for r, i in enumerate(image_ids):
        im = reconstruction.images[int(i)]
        pose[r] = im.cam_from_world.matrix()
        c = reconstruction.cameras[im.camera_id]
        prm = np.asarray(c.params, np.float64)
        if c.model_name not in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL"):
            raise NotImplementedError(f"camera model {c.model_name} is not supported (SIMPLE_PINHOLE, SIMPLE_RADIAL)")
        cam[r, :3] = prm[:3]
        cam[r, 3] = prm[3] if c.model_name == "SIMPLE_RADIAL" else 0.0
    return pose, cam


def sparse_order(reconstruction):
    """Host bookkeeping of the reference's loop (runner.py:757-770) over the reconstruction's point-major track CSR:
    (image ids in order of first appearance, per-output-row point row, image slot, point id, obs_ptr (S+1,))."""
    ptr, img, _ = reconstruction._track_csr()
    pid = np.repeat(np.arange(1, len(ptr), dtype=np.int64), np.diff(ptr))
    if len(img) == 0:
        return [], np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(1, np.int64)
    uniq, first = np.unique(img, return_index=True)
    image_ids = uniq[np.argsort(first, kind="stable")]                 # order of first appearance
    rank = np.empty(len(uniq), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    slot_of_row = rank[np.searchsorted(uniq, img)]
    order = np.argsort(slot_of_row, kind="stable")                      # stable partition by image
    counts = np.bincount(slot_of_row, minlength=len(uniq))
    obs_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [int(i) for i in image_ids], pid[order] - 1, slot_of_row[order], pid[order], obs_ptr


def sparse_depth(reconstruction, device=None):
    """:class:`SparseDepth` (names, obs_ptr (S+1,) numpy, uvd (O,3) and xyzid (O,4) float64 on the device)."""
    L = _lib.lib()
    dev = _dev(device)
    image_ids, prow, slot, pid, obs_ptr = sparse_order(reconstruction)
    O = len(prow)
    names = [reconstruction.images[i].name for i in image_ids]
    uvd = torch.empty((O, 3), dtype=torch.float64, device=dev)
    xyzid = torch.empty((O, 4), dtype=torch.float64, device=dev)
    if O:
        pose, cam = _camera_rows(reconstruction, image_ids)
        args = ((reconstruction._xyz[:reconstruction._n], np.float64), (prow, np.int32), (slot, np.int32), (pid, np.int64),
                (pose, np.float64), (cam, np.float64))
        _lib.check(L.vgg_sparse_depth(*[_to_dev(a, dt, dev) for a, dt in args], O, uvd, xyzid, _lib.stream_ptr()),
                   "vgg_sparse_depth")
    return SparseDepth(names, obs_ptr, uvd, xyzid)


def pack_maps(maps, device=None):
    """Ragged (H_i, W_i) float32 maps (numpy or torch) -> :class:`Packed` (one flat device buffer + int64 offsets and int32
    heights / widths on the device, max H*W)."""
    dev = _dev(device)
    shapes, parts = [], []
    for m in maps:
        if tuple(m.shape).__len__() != 2:
            raise ValueError(f"disparity maps must be 2-D (H, W), got shape {tuple(m.shape)}")
        dt = m.dtype
        if dt not in (np.float32, torch.float32):
            raise ValueError(f"disparity maps must be float32 (as the depth model writes them), got {dt}")
        shapes.append((int(m.shape[0]), int(m.shape[1])))
        parts.append(torch.as_tensor(m).reshape(-1))
    sizes = [h * w for h, w in shapes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = torch.cat([p.to(dev) for p in parts]) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
    hw = np.array(shapes, np.int32).reshape(-1, 2)
    return Packed(flat.contiguous(), torch.from_numpy(off).to(dev), torch.from_numpy(hw[:, 0].copy()).to(dev),
                  torch.from_numpy(hw[:, 1].copy()).to(dev), max(sizes) if sizes else 0)


def pack_samples(samples, num_images):
    """Recorded draws: a sequence (one (T_i, 2) array per image, in image order) -> (num_images, max T_i, 2) int32, rows
    past an image's own draws filled with -1 (reaching one is reported as status 6)."""
    if len(samples) != num_images:
        raise ValueError(f"samples: {len(samples)} entries for {num_images} images")
    arrs = [np.asarray(s, np.int64).reshape(-1, 2) for s in samples]
    T = max([len(a) for a in arrs] + [1])
    out = np.full((num_images, T, 2), -1, np.int32)
    for i, a in enumerate(arrs):
        if len(a) and (a.min() < 0 or a.max() >= 2 ** 31):
            raise ValueError("samples: draw indices must be non-negative int32")
        out[i, :len(a)] = a
    return out


def align(packed, uvd, obs_ptr, samples=None, seed=0, max_trials=MAX_TRIALS):
    """All images of `packed` at once (image i owns uvd rows obs_ptr[i]..obs_ptr[i+1]).  Returns :class:`AlignResult`
    with device tensors (per image: scale, shift float32, n_trials, n_inliers, n_kept, status int32; per observation:
    kept, inlier uint8)."""
    L = _lib.lib()
    dev = packed.flat.device
    S = len(obs_ptr) - 1
    O = int(obs_ptr[-1])
    if uvd.shape != (O, 3) or uvd.dtype != torch.float64 or not uvd.is_cuda:
        raise ValueError(f"uvd must be a ({O}, 3) float64 device tensor")
    if packed.off.numel() != S + 1:
        raise ValueError(f"{packed.off.numel() - 1} disparity maps for {S} images")
    if max_trials < 0:
        raise ValueError("max_trials must be >= 0")
    f32 = lambda: torch.zeros(S, dtype=torch.float32, device=dev)
    i32 = lambda: torch.zeros(S, dtype=torch.int32, device=dev)
    res = AlignResult(f32(), f32(), i32(), i32(), i32(), i32(), torch.zeros(O, dtype=torch.uint8, device=dev),
                      torch.zeros(O, dtype=torch.uint8, device=dev))
    if S == 0:
        return res
    draws, T = None, 0
    if samples is not None:
        d = samples if isinstance(samples, np.ndarray) and samples.ndim == 3 else pack_samples(samples, S)
        if d.shape[0] != S or d.shape[2] != 2:
            raise ValueError(f"samples must be (num_images={S}, T, 2), got {d.shape}")
        draws = _to_dev(d, np.int32, dev)
        T = d.shape[1]
    ptr_t = _to_dev(obs_ptr, np.int64, dev)
    nbytes = L.vgg_depth_align_workspace_bytes(O)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.vgg_depth_align(packed.flat, packed.off, packed.heights, packed.widths, uvd, ptr_t, S, O, draws, T,
                                 int(seed) & (2 ** 64 - 1), int(min(max_trials, 2 ** 31 - 1)), *res, ws, nbytes,
                                 _lib.stream_ptr()), "vgg_depth_align")
    return res


def apply(packed, scale, shift, num_images=None):
    """Rescale / validate / invert the first `num_images` maps of `packed` in place -> flat float32 depth (same layout)."""
    L = _lib.lib()
    S = packed.off.numel() - 1 if num_images is None else int(num_images)
    depth = torch.zeros_like(packed.flat)
    if S > 0:
        _lib.check(L.vgg_depth_apply(packed.flat, depth, packed.off, packed.heights, packed.widths, S, packed.max_pixels,
                                     scale, shift, _lib.stream_ptr()), "vgg_depth_apply")
    return depth


def unproject(packed, depth, cam, inv_pose, num_images=None):
    """World points (N,3) float64 of the valid pixels (disparity != 0 after :func:`apply`) of the first `num_images`
    images, image-major and row-major inside an image, plus the per-image counts (device int64)."""
    L = _lib.lib()
    S = packed.off.numel() - 1 if num_images is None else int(num_images)
    dev = packed.flat.device
    end = packed.off[S]
    pix = torch.nonzero(packed.flat[:end] != 0).reshape(-1)
    img = (torch.searchsorted(packed.off[1:S + 1], pix, right=True)).to(torch.int32)
    local = pix - packed.off[img.long()]
    counts = torch.bincount(img.long(), minlength=S)[:S]
    N = pix.numel()
    xyz = torch.empty((N, 3), dtype=torch.float64, device=dev)
    if N:
        cam_t, inv_t = _to_dev(cam, np.float64, dev), _to_dev(inv_pose, np.float64, dev)
        _lib.check(L.vgg_depth_unproject(local, img, N, depth, packed.off, packed.widths, cam_t, inv_t, xyz,
                                         _lib.stream_ptr()), "vgg_depth_unproject")
    return xyz, counts


def raise_for_status(code):
    """The reference's errors for a failed image (utils.py:661, 694; scikit-learn's for no consensus set)."""
    code = int(code)
    if code in (1, 4):
        raise ValueError("Too few points for depth alignment")
    if code == 2:
        raise ValueError("Ill-posed scene for depth alignment")
    if code == 3:
        raise ValueError("RANSAC could not find a valid consensus set. All `max_trials` iterations were skipped because "
                         "each randomly chosen sub-sample failed the passing criteria.")
    if code in (5, 6):
        raise ValueError(f"depth alignment: {ALIGN_STATUS[code]} (samples= does not cover the RANSAC loop)")
    if code != 0:
        raise RuntimeError(f"vgg_depth_align: unknown status {code}")
