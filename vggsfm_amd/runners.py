"""The part of ``VGGSfMRunner.sparse_reconstruct`` that follows the tracker (vggsfm/runners/runner.py:467-625), on the
device: two-view stage -> Triangulator -> optional dense extra points -> frame filtering / re-ordering -> back to the
original resolution -> the ``predictions`` dict the rest of the runner (saving, visualisation, dense depth) reads.

The learned parts stay with the caller: ``pred_cameras`` comes from the camera predictor (None: the cameras are built from
the tracks, ``vggsfm_amd.two_view_geo.geometric_camera_prior``), ``pred_track`` / ``pred_vis``
/ ``pred_score`` from the tracker, and the dense pass asks the caller's tracker for the grid tracks through
``extra_tracker`` (the reference calls ``predict_tracks`` there, runner.py:676-694).  Option names are the reference's
cfg keys (cfgs/demo.yaml)."""
from dataclasses import dataclass

import numpy as np
import torch

from .models import Triangulator
from .models.utils import sample_features4d
from .two_view_geo import estimate_preliminary_cameras
from .utils.triangulation import triangulate_extra_points


@dataclass
class GeometryConfig:
    fmat_thres: float = 4.0
    BA_iters: int = 2
    shared_camera: bool = False
    max_reproj_error: float = 4.0
    init_max_reproj_error: float = 4.0
    extract_color: bool = True
    robust_refine: int = 2
    camera_type: str = "SIMPLE_PINHOLE"
    extra_pt_pixel_interval: int = -1
    extra_by_neighbor: int = -1
    concat_extra_points: bool = False
    filter_invalid_frame: bool = True
    shift_point2d_to_original_res: bool = False
    max_ransac_iters: int = 4096
    lo_num: int = 300
    visual_dense_point_cloud: bool = False
    visual_tracks: bool = False


def generate_grid_samples(rect, N=None, pixel_interval=None):
    """vggsfm/utils/utils.py:773-815: (N,2) grid inside rect (1,4) = [x0, y0, x1, y1]; either N points at the rectangle's
    aspect ratio or one every `pixel_interval` pixels (x-major order)."""
    x0, y0, x1, y1 = (float(v) for v in rect[0])
    width, height = x1 - x0, y1 - y0
    if pixel_interval is not None:
        nx, ny = max(1, int(width // pixel_interval)), max(1, int(height // pixel_interval))
    else:
        nx = int(np.sqrt(N * (width / height)))
        ny = int(N / nx)
    gx, gy = torch.meshgrid(torch.linspace(x0, x1, nx, device=rect.device), torch.linspace(y0, y1, ny, device=rect.device),
                            indexing="ij")
    return torch.stack([gx.flatten(), gy.flatten()], dim=-1)


def sample_subrange(N, idx, L):
    """vggsfm/utils/utils.py:818-839: a window of L frames around idx, shifted to stay inside [0, N)."""
    start = idx - L // 2
    end = start + L
    if start < 0:
        end -= start
        start = 0
    if end > N:
        start = max(0, start - (end - N))
        end = N
    if end - start < L:
        if end < N:
            end = min(N, start + L)
        elif start > 0:
            start = max(0, end - L)
    return start, end


def rename_colmap_recons_and_rescale_camera(reconstruction, image_paths, crop_params, img_size,
                                            shift_point2d_to_original_res=False, shared_camera=False):
    """``VGGSfMRunner.rename_colmap_recons_and_rescale_camera`` (runner.py:1009-1054) over the pycolmap object surface:
    images get their file names; cameras go back to the original resolution -- focal x max(real size) / img_size,
    principal point = real size // 2, width / height = real size (only the first camera met when `shared_camera`,
    whose ratio then serves every image, as in the reference); optionally the 2D points too:
    (xy - |crop top-left|) x ratio, one array operation per image.  crop_params (1,S,>=4) tensor:
    [..., :2] real (w, h), [..., -4:-2] crop top-left."""
    cp = crop_params.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(crop_params) else np.asarray(crop_params, np.float64)
    rescale_camera, resize_ratio = True, None
    for image_id in reconstruction.images:
        image = reconstruction.images[image_id]
        camera = reconstruction.cameras[image.camera_id]
        image.name = image_paths[image_id]
        if rescale_camera:
            real = cp[0, image_id, :2]
            resize_ratio = float(real.max() / img_size)
            params = camera.params.copy()
            params[0] = resize_ratio * params[0]
            params[1:3] = real // 2
            camera.params = params
            camera.width, camera.height = real[0], real[1]
        if shift_point2d_to_original_res:
            top_left = np.abs(cp[0, image_id, -4:-2])
            image.points2D._xy[:] = (image.points2D._xy - top_left[None]) * resize_ratio
        if shared_camera:
            rescale_camera = False
    return reconstruction


class GeometryRunner:
    def __init__(self, cfg=None, triangulator=None):
        self.cfg = cfg or GeometryConfig()
        self.triangulator = triangulator or Triangulator()

    # ------------------------------------------------------------------ dense extra points (runner.py:627-742)
    def triangulate_extra_points(self, images, bound_bboxes, intrinsics, extra_params, extrinsics, image_paths, frame_num,
                                 extra_tracker):
        """For every frame: a pixel grid inside its bounding box is tracked through the neighbouring frames by
        `extra_tracker(frame_idx, neighbor_start, neighbor_end, grid_points (1,G,2)) -> (track (1,S',G,2), vis, score)`,
        triangulated with the refined cameras and filtered.  Returns {image_path: {points3D, points3D_rgb, uv}}."""
        cfg = self.cfg
        out = {}
        for frame_idx in range(frame_num):
            rect = bound_bboxes[:, frame_idx].clone().floor()
            rect[:, :2] += cfg.extra_pt_pixel_interval // 2
            rect[:, 2:] -= cfg.extra_pt_pixel_interval // 2
            grid = generate_grid_samples(rect, pixel_interval=cfg.extra_pt_pixel_interval).floor()
            grid_rgb = sample_features4d(images[:, frame_idx], grid[None]).squeeze(0)
            n0, n1 = sample_subrange(frame_num, frame_idx, cfg.extra_by_neighbor) if cfg.extra_by_neighbor > 0 else (0, frame_num)
            track, vis, score = extra_tracker(frame_idx, n0, n1, grid[None])
            ep = None if extra_params is None else extra_params[n0:n1]
            pts, valid = triangulate_extra_points(track.squeeze(0), vis.squeeze(0), score.squeeze(0), extrinsics[n0:n1],
                                                  intrinsics[n0:n1], ep, max_reproj_error=cfg.max_reproj_error)
            out[image_paths[frame_idx]] = {"points3D": pts[valid], "points3D_rgb": grid_rgb[valid], "uv": grid[valid]}
        return out

    # ------------------------------------------------------------------ runner.py:467-625
    def sparse_reconstruct_from_tracks(self, pred_cameras, pred_track, pred_vis, pred_score, images, crop_params=None,
                                       image_paths=None, center_order=None, back_to_original_resolution=True,
                                       extra_tracker=None, bound_bboxes=None, masks=None):
        cfg = self.cfg
        B, S, _, H, W = images.shape
        device = pred_track.device
        predictions = {}
        if image_paths is None:
            image_paths = [f"image_{s}" for s in range(S)]
        _, preliminary_dict = estimate_preliminary_cameras(pred_track, pred_vis, W, H, tracks_score=pred_score,
                                                           decompose=pred_cameras is None,    # (None: the prior needs them)
                                                           max_error=cfg.fmat_thres, loopresidual=True,
                                                           max_ransac_iters=cfg.max_ransac_iters, lo_num=cfg.lo_num)
        (extrinsics_opencv, intrinsics_opencv, extra_params, points3D, points3D_rgb, reconstruction, valid_frame_mask,
         valid_2D_mask, valid_tracks) = self.triangulator(
            pred_cameras, pred_track, pred_vis, images, preliminary_dict, pred_score=pred_score, BA_iters=cfg.BA_iters,
            shared_camera=cfg.shared_camera, max_reproj_error=cfg.max_reproj_error,
            init_max_reproj_error=cfg.init_max_reproj_error, extract_color=cfg.extract_color,
            robust_refine=cfg.robust_refine, camera_type=cfg.camera_type)
        additional_points_dict = None
        if cfg.extra_pt_pixel_interval > 0:
            if extra_tracker is None or bound_bboxes is None:
                raise ValueError("extra_pt_pixel_interval > 0 needs extra_tracker and bound_bboxes")
            additional_points_dict = self.triangulate_extra_points(images, bound_bboxes, intrinsics_opencv, extra_params,
                                                                   extrinsics_opencv, image_paths, S, extra_tracker)
            add_xyz = torch.cat([additional_points_dict[n]["points3D"] for n in image_paths], dim=0)
            add_rgb = torch.cat([additional_points_dict[n]["points3D_rgb"] for n in image_paths], dim=0)
            additional_points_dict["sfm_points_num"] = len(points3D)
            additional_points_dict["additional_points_num"] = len(add_xyz)
            if cfg.concat_extra_points:              # runner.py:549-559, all points at once (empty tracks)
                reconstruction.add_points3D(add_xyz.cpu().numpy(), (add_rgb * 255).long().cpu().numpy())
                points3D = torch.cat([points3D, add_xyz.to(points3D.dtype)], dim=0)
                points3D_rgb = torch.cat([points3D_rgb, add_rgb.to(points3D_rgb.dtype)], dim=0)
        if cfg.filter_invalid_frame:
            extrinsics_opencv = extrinsics_opencv[valid_frame_mask]
            intrinsics_opencv = intrinsics_opencv[valid_frame_mask]
            if extra_params is not None:
                extra_params = extra_params[valid_frame_mask]
            for invalid_id in torch.nonzero(~valid_frame_mask).squeeze(1).cpu().tolist():
                reconstruction.deregister_image(invalid_id)
        img_size = images.shape[-1]
        if center_order is not None:                       # the images were re-ordered around the query frame: undo it
            extrinsics_opencv = extrinsics_opencv[center_order]
            intrinsics_opencv = intrinsics_opencv[center_order]
            if extra_params is not None:
                extra_params = extra_params[center_order]
            pred_track = pred_track[:, center_order]
            pred_vis = pred_vis[:, center_order]
            if pred_score is not None:
                pred_score = pred_score[:, center_order]
        if back_to_original_resolution:
            if crop_params is None:
                raise ValueError("back_to_original_resolution needs crop_params")
            reconstruction = rename_colmap_recons_and_rescale_camera(
                reconstruction, image_paths, crop_params, img_size, shared_camera=cfg.shared_camera,
                shift_point2d_to_original_res=cfg.shift_point2d_to_original_res)
            # intrinsics at the original resolution, in the order of the sorted image paths (runner.py:593-608)
            fname_to_id = {reconstruction.images[i].name: i for i in reconstruction.images}
            K = [reconstruction.cameras[reconstruction.images[fname_to_id[n]].camera_id].calibration_matrix()
                 for n in sorted(image_paths)]
            intrinsics_opencv = torch.from_numpy(np.stack(K)).to(device)
        predictions.update(extrinsics_opencv=extrinsics_opencv, intrinsics_opencv=intrinsics_opencv, points3D=points3D,
                           points3D_rgb=points3D_rgb, reconstruction=reconstruction, extra_params=extra_params,
                           unproj_dense_points3D=None, valid_2D_mask=valid_2D_mask, pred_track=pred_track, pred_vis=pred_vis,
                           pred_score=pred_score, valid_tracks=valid_tracks, additional_points_dict=additional_points_dict,
                           preliminary_dict=preliminary_dict)
        return predictions

    # ------------------------------------------------------------------ frames in, reconstruction out (no learned part)
    def reconstruct_from_frames(self, images, query_frame=0, max_query_pts=2048, bound_bboxes=None, **tracker_options):
        """The whole sparse reconstruction from frames alone: images (1,S,3,H,W) float32 in [0, 1] -> the corners of
        `query_frame` tracked through the sequence (vggsfm_amd.klt.KLTTracker, `tracker_options` are its options) ->
        sparse_reconstruct_from_tracks without predicted cameras, at the resolution of the frames.  With
        cfg.extra_pt_pixel_interval > 0 the tracker also serves the dense extra points (bound_bboxes (1,S,4), default: the
        whole frame).  predictions["tracker"] keeps the tracker."""
        from .klt import KLTTracker

        if images.dim() == 4:
            images = images[None]
        S, H, W = images.shape[1], images.shape[-2], images.shape[-1]
        tracker = KLTTracker(images, **tracker_options)
        pred_track, pred_vis, pred_score = tracker.predict_tracks(query_frame=query_frame, max_query_pts=max_query_pts)
        extra = None
        if self.cfg.extra_pt_pixel_interval > 0:
            extra = tracker.extra_tracker
            if bound_bboxes is None:
                bound_bboxes = torch.tensor([0.0, 0.0, W - 1.0, H - 1.0], device=images.device).expand(1, S, 4)
        predictions = self.sparse_reconstruct_from_tracks(None, pred_track, pred_vis, pred_score, images,
                                                          back_to_original_resolution=False, extra_tracker=extra,
                                                          bound_bboxes=bound_bboxes)
        predictions["tracker"] = tracker
        return predictions

    # ------------------------------------------------------------------ dense depth (runner.py:744-814)
    def extract_sparse_depth_and_point_from_reconstruction(self, predictions):
        """runner.py:744-772 with one projection kernel (vgg_sparse_depth) instead of the per-observation loop.  Sets
        predictions["sparse_depth"] / ["sparse_point"]: per image name (in order of first appearance) an (n,3) array of
        [u, v, depth] and an (n,4) array of [x, y, z, point3D_id], float64 (the reference keeps lists of 1-D arrays;
        ``np.array`` of either is the same).  predictions["sparse_depth_device"] keeps the device-side result
        (vggsfm_amd.dense_depth.SparseDepth) for ``dense_reconstruct``."""
        from collections import defaultdict

        from . import dense_depth as DD

        sd = DD.sparse_depth(predictions["reconstruction"])
        uvd, xyzid = sd.uvd.cpu().numpy(), sd.xyzid.cpu().numpy()
        sparse_depth, sparse_point = defaultdict(list), defaultdict(list)
        for k, name in enumerate(sd.names):
            a, b = int(sd.obs_ptr[k]), int(sd.obs_ptr[k + 1])
            sparse_depth[name] = uvd[a:b]
            sparse_point[name] = xyzid[a:b]
        predictions["sparse_depth"] = sparse_depth
        predictions["sparse_point"] = sparse_point
        predictions["sparse_depth_device"] = sd
        return predictions

    def dense_reconstruct(self, predictions, image_paths, original_images, disp_dict, samples=None, generator=None):
        """runner.py:776-814 without the depth network: `disp_dict` holds the monocular disparity maps the caller's model
        predicted (float32 (H, W) numpy arrays or device tensors, keyed by image name, as extract_dense_depth_maps returns
        them); they are rescaled in place.  Sets predictions["depth_dict"] and ["unproj_dense_points3D"]
        (cfg.visual_dense_point_cloud)."""
        from .utils.utils import align_dense_depth_maps

        depth_dict, unproj = align_dense_depth_maps(
            predictions["reconstruction"], predictions["sparse_depth"], disp_dict, original_images,
            visual_dense_point_cloud=bool(getattr(self.cfg, "visual_dense_point_cloud", False)), samples=samples,
            generator=generator)
        predictions["depth_dict"] = depth_dict
        predictions["unproj_dense_points3D"] = unproj
        return predictions

    # ------------------------------------------------------------------ dense depth from frames (no learned part)
    def dense_reconstruct_from_frames(self, predictions, images, original_images=None, **options):
        """The dense stage for users without a depth network: every registered image of predictions["reconstruction"] is
        swept against its neighbours by plane-sweep stereo and checked against their maps (vggsfm_amd.mvs, `options` are
        dense_depth_from_frames').  images: the frames the reconstruction was made from, (S,3,H,W) or (1,S,3,H,W) float32
        in [0, 1], frame i belonging to image id i.  Sets predictions["depth_dict"] and ["depth_conf_dict"] ((H,W) float32
        device tensors by image name, depth 0 = none) and, with cfg.visual_dense_point_cloud,
        ["unproj_dense_points3D"] in align_dense_depth_maps' format: per name np.array([xyz, rgb]), the colours from
        original_images[name] ((H,W,3), 0 .. 255) or, without them, from the frames.

        Option patchmatch_iterations (default 0: the sweep alone, as before): with more, the swept maps are refined by
        that many PatchMatch slanted-plane iterations before the check (vggsfm_amd.patchmatch, whose
        dense_depth_from_frames then takes `options`, `seed` among them), and predictions["depth_normal_dict"] holds the
        unit world normals ((H,W,3) float32 device tensors by image name, (0, 0, 0) = none)."""
        from . import mvs

        rec = predictions["reconstruction"]
        patchmatch_iterations = int(options.pop("patchmatch_iterations", 0))
        if patchmatch_iterations > 0:
            from . import patchmatch

            depth_dict, conf_dict, normal_dict = patchmatch.dense_depth_from_frames(rec, images, patchmatch_iterations, **options)
            predictions["depth_normal_dict"] = normal_dict
        else:
            depth_dict, conf_dict = mvs.dense_depth_from_frames(rec, images, **options)
        predictions["depth_dict"] = depth_dict
        predictions["depth_conf_dict"] = conf_dict
        unproj = None
        if bool(getattr(self.cfg, "visual_dense_point_cloud", False)):
            unproj = {}
            xyz = mvs.unproject_depth_maps(rec, depth_dict)
            frames = images[0] if images.dim() == 5 else images
            by_name = {rec.images[i].name: i for i in rec.images}
            for name, depth in depth_dict.items():
                valid = (depth != 0).reshape(-1).cpu().numpy()
                if original_images is not None:
                    img = original_images[name]
                    img = img.cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
                    rgb = (img / 255.0).reshape(-1, 3)[valid]
                else:
                    f = frames[by_name[name]]
                    f = f.expand(3, *f.shape[-2:]) if f.dim() == 2 or f.shape[0] == 1 else f
                    rgb = f.permute(1, 2, 0).reshape(-1, 3).double().cpu().numpy()[valid]
                unproj[name] = np.array([xyz[name].cpu().numpy(), rgb])
        predictions["unproj_dense_points3D"] = unproj
        return predictions

    # ------------------------------------------------------------------ one fused cloud from the depth maps
    def fuse_dense_point_cloud(self, predictions, images, output_path=None, **options):
        """The last stage of the dense path: predictions["depth_dict"] (of dense_reconstruct_from_frames or
        align_dense_depth_maps, (H,W) float32 device tensors by image name) fused into ONE cloud in the gauge of
        predictions["reconstruction"] (vggsfm_amd.fusion, `options` are fuse_reconstruction's).  images: the frames, frame
        i belonging to image id i, for the colours; None: no colours.  Sets predictions["fused_point_cloud"], a
        fusion.FusedCloud of device tensors (xyz, normal, rgb, num_views, view = image id, pixel) with each surface point
        once; with `output_path` the cloud is also written there as a binary PLY.  No other key changes."""
        from . import fusion

        cloud = fusion.fuse_reconstruction(predictions["reconstruction"], predictions["depth_dict"], images, **options)
        predictions["fused_point_cloud"] = cloud
        if output_path is not None:
            fusion.write_ply(output_path, cloud)
        return predictions

    # ------------------------------------------------------------------ one surface from the depth maps
    def mesh_dense_surface(self, predictions, images=None, output_path=None, confidence_weights=False, **options):
        """The surface of the dense path: predictions["depth_dict"] integrated into a TSDF volume and its zero level set
        extracted as a triangle mesh in the gauge of predictions["reconstruction"] (vggsfm_amd.meshing, `options` are
        mesh_reconstruction's: resolution, margin, trunc, min_weight, bounds).  images: the frames, frame i belonging to
        image id i, for the colours; None: no colours.  confidence_weights: weigh every pixel by
        predictions["depth_conf_dict"] instead of 1.  Sets predictions["dense_mesh"], a meshing.Mesh of device tensors
        (vertices, normals, rgb, faces); with `output_path` the mesh is also written there as a binary PLY.  No other key
        changes."""
        from . import meshing

        conf = predictions["depth_conf_dict"] if confidence_weights else None
        mesh = meshing.mesh_reconstruction(predictions["reconstruction"], predictions["depth_dict"], images, conf, **options)
        predictions["dense_mesh"] = mesh
        if output_path is not None:
            meshing.write_mesh_ply(output_path, mesh)
        return predictions

    # ------------------------------------------------------------------ the surface seen from the cameras
    def render_dense_mesh(self, predictions, **options):
        """predictions["dense_mesh"] (of mesh_dense_surface) rendered into every registered image of
        predictions["reconstruction"] through a z-buffer (vggsfm_amd.render, `options` are render_reconstruction's).  Sets
        predictions["mesh_depth_dict"] ((H,W) float32 device tensors by image name, 0 = none: hole-free wherever the mesh
        is, and occlusion-correct), ["mesh_normal_dict"] and ["mesh_rgb_dict"] ((H,W,3) float32: the mesh's unit world
        normals and colours, zeros = none) -- the shapes depth_dict and depth_normal_dict use.  No other key changes."""
        from . import render

        depth, normal, rgb, _ = render.render_reconstruction(predictions["reconstruction"], predictions["dense_mesh"], **options)
        predictions["mesh_depth_dict"] = depth
        predictions["mesh_normal_dict"] = normal
        predictions["mesh_rgb_dict"] = rgb
        return predictions

    # ------------------------------------------------------------------ the dense model against a reference
    def evaluate_dense_model(self, predictions, reference, thresholds, max_dist, which="fused_point_cloud", transform=None):
        """How far predictions[which] -- "fused_point_cloud" (of fuse_dense_point_cloud) or "dense_mesh" (of
        mesh_dense_surface) -- is from `reference` (a point set (N,3), a fusion.FusedCloud or a meshing.Mesh in the same
        gauge, or in the gauge that `transform` = (scale, R, t) of vggsfm_amd.sim3 takes the prediction to): accuracy,
        completeness and, per threshold, precision, recall and F-score within max_dist (vggsfm_amd.utils.dense_metric).
        Sets predictions["dense_metrics"], a dict of Python numbers.  No other key changes."""
        from .utils import dense_metric

        if which not in ("fused_point_cloud", "dense_mesh"):
            raise ValueError(f"which must be 'fused_point_cloud' or 'dense_mesh', got {which!r}")
        predictions["dense_metrics"] = dense_metric.evaluate_dense(predictions[which], reference, thresholds, max_dist, transform)
        return predictions

    # ------------------------------------------------------------------ the dense model registered to a reference
    def register_dense_model(self, predictions, reference, max_dist, which="fused_point_cloud", init=None, **options):
        """predictions[which] -- "fused_point_cloud" or "dense_mesh" (its vertices) -- registered to `reference` (a point
        set (N,3), a fusion.FusedCloud, a meshing.Mesh or a registration.Target) by ICP on the dense geometry
        (vggsfm_amd.registration.icp, `options` are its keywords; max_dist a number or coarse-to-fine stages; init = (scale,
        R, t), e.g. of sim3.align_cameras).  A point set without normals gets them estimated within normal_radius (default:
        twice the last max_dist) unless metric="point_to_point".  Sets predictions["dense_registration"]: scale, R, t,
        transform = (scale, R, t) as device tensors, the tuple evaluate_dense_model(transform=...) takes, status, iterations,
        rmse, fitness.  No other key changes."""
        from . import registration

        if which not in ("fused_point_cloud", "dense_mesh"):
            raise ValueError(f"which must be 'fused_point_cloud' or 'dense_mesh', got {which!r}")
        stages = list(max_dist) if isinstance(max_dist, (list, tuple)) else [max_dist]
        normal_radius = options.pop("normal_radius", 2.0 * float(stages[-1]))
        if options.get("metric", "point_to_plane") == "point_to_point":
            normal_radius = None
        cell = options.get("cell") or float(stages[0])
        target = reference if isinstance(reference, registration.Target) else registration.make_target(reference, cell, normal_radius)
        model = predictions[which]
        reg = registration.icp(model, target, max_dist, init=init, **options)
        dev = target.grid.device
        transform = (torch.tensor(reg.scale, dtype=torch.float64, device=dev), reg.R.to(dev), reg.t.to(dev))
        predictions["dense_registration"] = {"scale": reg.scale, "R": reg.R, "t": reg.t, "transform": transform, "status": reg.status,
                                             "iterations": reg.iterations, "rmse": reg.rmse, "fitness": reg.fitness}
        return predictions

    # ------------------------------------------------------------------ track video (runner.py:445-450)
    def visualize_tracks(self, images, pred_track, pred_vis, output_dir=None):
        """runner.py:445-450 (cfg.visual_tracks): the tracker's raw predictions drawn over the frames, on the device
        (vggsfm_amd.utils.visualizer.Visualizer, linewidth 1).  images (1,S,3,H,W) in [0, 1], pred_track (1,S,N,2),
        pred_vis (1,S,N).  Returns the video (1, S + 2, 3, H, W) uint8 on the device; with `output_dir` it is also written
        to output_dir/visuals/track.mp4 (needs imageio, see Visualizer.save_video)."""
        import os

        from .utils.visualizer import Visualizer

        save_dir = "./results" if output_dir is None else os.path.join(output_dir, "visuals")
        vis = Visualizer(save_dir=save_dir, linewidth=1)
        return vis.visualize(images * 255, pred_track, pred_vis[..., None], filename="track", save_video=output_dir is not None)

    # ------------------------------------------------------------------ reprojection video (runner.py:834-885)
    def make_reprojection_video(self, predictions, video_size, image_paths, original_images):
        """runner.py:834-866: one padded BGR frame (numpy uint8) per image, in sorted-name order, with the visible sparse
        observations drawn (vggsfm_amd.utils.utils.create_video_with_reprojections).  Reads the device-side
        predictions["sparse_depth_device"] when extract_sparse_depth_and_point_from_reconstruction left it, so nothing of
        the sparse depth goes through the host; otherwise predictions["sparse_depth"] / ["sparse_point"].
        video_size: (width, height)."""
        import os

        from .utils.utils import create_video_with_reprojections

        sparse_depth = predictions.get("sparse_depth_device")
        if sparse_depth is None:
            sparse_depth = predictions["sparse_depth"]
        image_dir_prefix = os.path.dirname(image_paths[0])
        image_paths = [os.path.basename(p) for p in image_paths]
        return create_video_with_reprojections(image_dir_prefix, video_size, predictions["reconstruction"], image_paths,
                                               sparse_depth, predictions.get("sparse_point"), original_images)

    def save_reprojection_video(self, img_with_circles_list, video_size, output_dir):
        """runner.py:868-885: writes output_dir/visuals/reproj.mp4 (needs OpenCV, see save_video_with_reprojections)."""
        import os

        from .utils.utils import save_video_with_reprojections

        visual_dir = os.path.join(output_dir, "visuals")
        os.makedirs(visual_dir, exist_ok=True)
        save_video_with_reprojections(os.path.join(visual_dir, "reproj.mp4"), img_with_circles_list, video_size)
