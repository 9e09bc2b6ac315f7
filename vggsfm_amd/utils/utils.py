"""Camera-prediction averaging of the reference (vggsfm/utils/utils.py:25-187), as torch ops on the device, and its dense
depth alignment (``align_dense_depth_maps``, utils.py:635-770) over the kernels of vggsfm_amd/dense_depth.py, and its
reprojection video (``filter_invisible_reprojections``, ``create_video_with_reprojections``, utils.py:393-546) over the
kernels of vggsfm_amd/reproj_video.py.

``average_camera_prediction`` runs the (learned, injected) camera predictor several times, each time with a different
frame swapped to position 0, brings every prediction back to the frame order and to the gauge of frame 0, and averages:
rotations through the mean of their quaternions, translations and focal lengths arithmetically.  The reference does
the quaternion step on the host with scipy; here it stays on the device and follows scipy's conventions exactly
(``Rotation.from_matrix(...).as_quat()`` of scipy 1.15: SVD orthogonalisation of non-orthogonal input, x,y,z,w,
largest-component branch, no sign canonicalisation) so that the mean
-- which is sign sensitive -- is the reference's.  Used by ``VGGSfMRunner.sparse_reconstruct`` (cfg.avg_pose,
runner.py:392-400) and by the video runner for every window (video_runner.py:662-667): ``VideoGeometry``'s default
``camera_prior`` (``camera_prior_from_predictor``).
"""
import random
import types

import numpy as np
import torch


def calculate_index_mappings(query_index, S, device=None):
    """Order that swaps [query_index] and [0] (utils.py:167-177)."""
    new_order = torch.arange(S)
    new_order[0] = query_index
    new_order[query_index] = 0
    return new_order if device is None else new_order.to(device)


def switch_tensor_order(tensors, order, dim=1):
    """utils.py:180-187."""
    return [torch.index_select(t, dim, order) if t is not None else None for t in tensors]


def closed_form_inverse_OpenCV(se3):
    """[R t; 0 1]^-1 = [R^T  -R^T t; 0 1] for a batch of 4x4 matrices (utils/metric.py:233-268)."""
    R, T = se3[:, :3, :3], se3[:, :3, 3:]
    Rt = R.transpose(1, 2)
    inv = torch.eye(4, dtype=se3.dtype, device=se3.device)[None].repeat(len(se3), 1, 1)
    inv[:, :3, :3] = Rt
    inv[:, :3, 3:] = -Rt.bmm(T)
    return inv


def matrix_to_quaternion_scipy(M):
    """(...,3,3) -> (...,4) quaternion (x,y,z,w) with scipy's ``Rotation.from_matrix`` branch structure and sign: the largest
    of (m00, m11, m22, trace) selects the formula; unit norm; the sign is whatever the formula gives."""
    M = M.to(torch.float64)
    # scipy >= 1.11 first orthogonalises an input whose Gramian is not the identity to np.isclose(atol=1e-12) -- every
    # float32 prediction -- by the orthogonal Procrustes solution U V^T of its SVD
    G = M @ M.transpose(-1, -2)
    eye = torch.eye(3, dtype=M.dtype, device=M.device)
    off = ((G - eye).abs() > 1e-12 + 1e-5 * eye).any(-1).any(-1)
    if bool(off.any()):
        U, _, Vh = torch.linalg.svd(M)
        M = torch.where(off[..., None, None], U @ Vh, M)
    m = lambda a, b: M[..., a, b]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    dec = torch.stack([m(0, 0), m(1, 1), m(2, 2), tr], -1)
    choice = dec.argmax(-1)
    cands = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        q = [None] * 4
        q[i] = 1 - dec[..., 3] + 2 * m(i, i)
        q[j] = m(j, i) + m(i, j)
        q[k] = m(k, i) + m(i, k)
        q[3] = m(k, j) - m(j, k)
        cands.append(torch.stack(q, -1))
    cands.append(torch.stack([m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1), 1 + dec[..., 3]], -1))
    q = torch.gather(torch.stack(cands, -2), -2, choice[..., None, None].expand(choice.shape + (1, 4))).squeeze(-2)
    return q / q.norm(dim=-1, keepdim=True)


def quaternion_to_matrix_scipy(q):
    """(...,4) unit quaternion (x,y,z,w) -> (...,3,3), scipy's ``Rotation.from_quat(...).as_matrix()`` formula."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    R = torch.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw),
                     2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw),
                     2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def average_batch_rotation_matrices(batch_rotation_matrices):
    """(B,N,3,3) -> (N,3,3): normalised mean of the quaternions over B (utils.py:136-164), float64."""
    q = matrix_to_quaternion_scipy(batch_rotation_matrices).mean(0)
    q = q / q.norm(dim=1, keepdim=True)
    # scipy normalises once more inside from_quat
    return quaternion_to_matrix_scipy(q / q.norm(dim=1, keepdim=True))


def average_camera_prediction(camera_predictor, reshaped_image, batch_size, repeat_times=5, query_indices=None):
    """utils.py:25-127.  `camera_predictor(images, batch_size=...)["pred_cameras"]` must expose ``R`` (S,3,3), ``T`` (S,3)
    and ``focal_length`` (S,2) in the OpenCV convention.  Returns a camera object of the predictor's own type when it
    can be built from (focal_length, R, T, device), else a namespace with those three fields."""
    assert batch_size == 1, "This function is designed for inference with batch_size=1."
    num_frames = len(reshaped_image)
    device = reshaped_image.device
    if query_indices is None:
        repeat_times = min(repeat_times, num_frames)
        query_indices = random.sample(range(num_frames), repeat_times)
        if 0 not in query_indices:
            query_indices.insert(0, 0)
    rotations, translations, focal_lengths = [], [], []
    pred_cameras = None
    for query_index in query_indices:
        new_order = calculate_index_mappings(query_index, num_frames, device=device)
        ordered = switch_tensor_order([reshaped_image], new_order, dim=0)[0]
        pred_cameras = camera_predictor(ordered, batch_size=batch_size)["pred_cameras"]
        R, abs_T = pred_cameras.R, pred_cameras.T
        ext = torch.eye(4, dtype=R.dtype, device=R.device)[None].repeat(len(R), 1, 1)
        ext[:, :3, :3] = R
        ext[:, :3, 3] = abs_T
        ext, focal = switch_tensor_order([ext, pred_cameras.focal_length], new_order, dim=0)
        rel = closed_form_inverse_OpenCV(ext[0:1]).expand(len(ext), -1, -1)
        ext = torch.bmm(ext, rel)                     # relative to the first camera (OpenCV convention: right-multiply)
        rotations.append(ext[:, :3, :3][None])
        translations.append(ext[:, :3, 3][None])
        focal_lengths.append(focal[None])
    avg_R = average_batch_rotation_matrices(torch.cat(rotations))
    avg_T = torch.cat(translations).mean(0)
    avg_f = torch.cat(focal_lengths).mean(0)
    try:
        return type(pred_cameras)(focal_length=avg_f, R=avg_R, T=avg_T, device=device)
    except TypeError:
        return types.SimpleNamespace(focal_length=avg_f, R=avg_R, T=avg_T, device=device)


def camera_prior_from_predictor(camera_predictor, images):
    """The ``camera_prior`` callable ``VideoGeometry.move_window`` takes, as the reference builds it
    (video_runner.py:655-681): averaged prediction over the frames [frame_from, frame_to) of `images` (1,S,3,H,W) with
    the query frames (first, middle, last) -> (frame_to - frame_from, 3, 4) extrinsics in the predictor's own gauge."""
    def prior(frame_from, frame_to):
        window = images[:, frame_from:frame_to]
        n = window.shape[1]
        cams = average_camera_prediction(camera_predictor, window.reshape((-1,) + tuple(window.shape[2:])), 1,
                                         query_indices=[0, n // 2, n - 1])
        return torch.cat((cams.R, cams.T.unsqueeze(-1)), dim=-1)
    return prior


def align_dense_depth_maps(reconstruction, sparse_depth, disp_dict, original_images, visual_dense_point_cloud=False,
                           samples=None, generator=None, device=None):
    """utils.py:635-770 on the device (vggsfm_amd/dense_depth.py, csrc/dense.hip): per key of `sparse_depth` (in its
    order) the RANSAC fit disparity ~ scale * (1 / depth) + shift, then every map of `disp_dict` is rescaled IN PLACE,
    validated to (0, 1e4] and inverted.  Returns (depth_dict, unproj_dense_points3D or None) like the reference, and raises
    its ValueErrors -- after the maps of the images before the failing one were rescaled, as the reference's loop leaves
    them.

    disp_dict values: float32 (H, W) numpy arrays (depth_dict then holds numpy float32 maps) or float32 device tensors
    (depth_dict holds device tensors, nothing is copied to the host except the dense cloud).  `samples`: recorded
    scikit-learn draws, one (T, 2) index array per key (a sequence in key order or a dict by key), replayed exactly;
    otherwise the draws come from a generator on the device seeded from `generator` (torch.Generator, int or None)."""
    from .. import dense_depth as DD

    names = list(sparse_depth)
    if not names:
        return {}, ({} if visual_dense_point_cloud else None)
    dev = torch.device("cuda" if device is None else device)
    uvds = [np.asarray(sparse_depth[n], dtype=np.float64).reshape(-1, 3) for n in names]
    obs_ptr = np.concatenate([[0], np.cumsum([len(u) for u in uvds])]).astype(np.int64)
    maps = [disp_dict[n] for n in names]
    on_device = all(torch.is_tensor(m) for m in maps)
    packed = DD.pack_maps(maps, dev)
    uvd = torch.from_numpy(np.concatenate(uvds) if obs_ptr[-1] else np.zeros((0, 3))).to(dev)
    if isinstance(samples, dict):
        samples = [samples[n] for n in names]
    if isinstance(generator, int):
        seed = generator
    else:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    res = DD.align(packed, uvd, obs_ptr, samples=samples, seed=seed)
    status = res.status.cpu().numpy()
    bad = np.nonzero(status != 0)[0]
    n_ok = int(bad[0]) if len(bad) else len(names)
    depth = DD.apply(packed, res.scale, res.shift, n_ok)
    off = packed.off.cpu().numpy()
    depth_dict, cloud = {}, {}
    if visual_dense_point_cloud and n_ok:
        ids = {reconstruction.images[i].name: i for i in reconstruction.images}
        img_ids = [ids[n] for n in names[:n_ok]]
        pose, cam = DD._camera_rows(reconstruction, img_ids)
        inv = [reconstruction.images[i].cam_from_world.inverse() for i in img_ids]     # [R^T | -R^T t] as Rigid3d
        inv_pose = np.stack([np.concatenate([t.rotation.matrix(), t.translation[:, None]], axis=1) for t in inv])
        xyz, counts = DD.unproject(packed, depth, cam, inv_pose, n_ok)
        xyz = xyz.cpu().numpy()
        cstart = np.concatenate([[0], np.cumsum(counts.cpu().numpy())])
    flat_host = packed.flat.cpu() if not on_device else None
    depth_host = depth.cpu() if not on_device else None
    for k, n in enumerate(names[:n_ok]):
        h, w = maps[k].shape
        a, b = int(off[k]), int(off[k + 1])
        if on_device:
            maps[k].copy_(packed.flat[a:b].view(h, w))
            depth_dict[n] = depth[a:b].view(h, w).clone()
        else:
            maps[k][...] = flat_host[a:b].numpy().reshape(h, w)
            depth_dict[n] = depth_host[a:b].numpy().reshape(h, w).copy()
        if visual_dense_point_cloud:
            valid = (maps[k] != 0).reshape(-1)
            valid = valid.cpu().numpy() if torch.is_tensor(valid) else valid
            img = original_images[n]
            img = img.cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
            rgb = (img / 255.0).reshape(-1, 3)[valid]
            cloud[n] = np.array([xyz[cstart[k]:cstart[k + 1]], rgb])
    if len(bad):
        DD.raise_for_status(status[bad[0]])
    return depth_dict, (cloud if visual_dense_point_cloud else None)


def filter_invisible_reprojections(uvs_int, depths):
    """utils.py:393-425 on the device (vggsfm_amd/reproj_video.py, csrc/reproj.hip): True for every point that wins its
    integer pixel -- the smallest depth, ties to the lowest index, -0.0 == +0.0, a NaN depth first (np.argmin's rules).
    numpy in -> numpy bool mask out; device tensors in -> device bool mask out.  The device grid covers the points'
    bounding box: one of more than 2^27 pixels raises ValueError."""
    from ..reproj_video import filter_mask

    return filter_mask(uvs_int, depths)


def create_video_with_reprojections(fname_prefix, video_size, reconstruction, image_paths, sparse_depth, sparse_point,
                                    original_images=None, draw_radius=3, cmap="gist_rainbow", color_mode="dis_to_center",
                                    *, device=None):
    """utils.py:428-546 on the device (vggsfm_amd/reproj_video.py): one padded (H, W, 3) uint8 BGR numpy frame per name of
    ``sorted(image_paths)`` with the visible observations drawn as filled circles of radius `draw_radius` in the colour of
    their point (statistics, colours, centres, visibility and drawing order are the reference's exactly; the circles follow
    the integer raster rule of DESIGN.md section 12, not OpenCV's anti-aliasing).

    sparse_depth / sparse_point: the reference's dicts ({name: (n,3) [u, v, depth]} / {name: (n,4) [x, y, z, id]}), or
    `sparse_depth` = the device-side :class:`vggsfm_amd.dense_depth.SparseDepth` (`sparse_point` is then not read).
    original_images: {name: (h, w, 3) uint8 RGB} numpy arrays or device tensors; None reads ``fname_prefix/name`` with PIL
    (its decoder, not OpenCV's).  An image without observations is output undrawn (the reference raises IndexError).
    Raises NotImplementedError for an unknown `color_mode` and ValueError for a frame larger than `video_size` or a
    negative `draw_radius`, before anything is launched."""
    import os

    from .. import dense_depth as DD
    from .. import reproj_video as RV

    dev = torch.device("cuda" if device is None else device)
    names = sorted(image_paths)
    if original_images is None:
        from PIL import Image
        images = {n: np.asarray(Image.open(os.path.join(fname_prefix, n)).convert("RGB")) for n in names}
    else:
        images = {n: original_images[n] for n in names}
    RV._validate(images, video_size, draw_radius, color_mode)
    if isinstance(sparse_depth, DD.SparseDepth):
        sd = sparse_depth
    else:
        keys = list(sparse_depth)
        uvd = [np.asarray(sparse_depth[k], np.float64).reshape(-1, 3) for k in keys]
        xyzid = [np.asarray(sparse_point[k], np.float64).reshape(-1, 4) for k in keys]
        obs_ptr = np.concatenate([[0], np.cumsum([len(u) for u in uvd])]).astype(np.int64)
        cat = lambda a, c: torch.from_numpy(np.concatenate(a) if obs_ptr[-1] else np.zeros((0, c))).to(dev)
        sd = DD.SparseDepth(keys, obs_ptr, cat(uvd, 3), cat(xyzid, 4))
    xyz, ids = RV.live_points(reconstruction)
    frames = RV.render(sd, xyz, ids, images, video_size, draw_radius=draw_radius, cmap=cmap, color_mode=color_mode,
                       device=dev)
    host = frames.cpu().numpy()
    return [host[k] for k in range(len(names))]


def save_video_with_reprojections(output_path, img_with_circles_list, video_size, fps=1):
    """utils.py:549-571: the frames (BGR uint8, numpy or device tensors) as an mp4v video through OpenCV.  Encoding needs
    OpenCV (``cv2``); without it this raises ImportError."""
    try:
        import cv2
    except ImportError as e:
        raise ImportError("save_video_with_reprojections needs OpenCV (the cv2 module) to encode the video; install "
                          "opencv-python, or write the frames of create_video_with_reprojections yourself") from e
    writer = cv2.VideoWriter(output_path, cv2.VideoWriter_fourcc(*"mp4v"), fps, tuple(int(v) for v in video_size))
    for frame in img_with_circles_list:
        writer.write(frame.cpu().numpy() if torch.is_tensor(frame) else np.asarray(frame))
    writer.release()
