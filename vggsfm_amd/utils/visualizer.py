"""The reference's track visualizer (vggsfm/utils/visualizer.py) over the HIP track video
(:mod:`vggsfm_amd.track_video`): same class, same parameter lists, the drawing on the device.

What the runner's call (runner.py:445-450) does not use is not implemented and says so before anything is launched:
``mode="optical_flow"``, ``segm_mask``, ``gt_tracks``, ``compensate_for_camera_motion``, ``tracks_leave_trace != 0`` and
``grayscale=True`` raise NotImplementedError."""
import os

import torch

from .. import track_video as TV


class Visualizer:
    def __init__(
        self,
        save_dir: str = "./results",
        grayscale: bool = False,
        pad_value: int = 0,
        fps: int = 1,
        mode: str = "rainbow",  # 'cool'
        linewidth: int = 1,
        show_first_frame: int = 3,
        tracks_leave_trace: int = 0,
    ):
        TV.check_options(mode=mode, grayscale=grayscale, tracks_leave_trace=tracks_leave_trace)
        TV.radius_of(linewidth)
        self.mode = mode
        self.save_dir = save_dir
        self.show_first_frame = show_first_frame
        self.grayscale = grayscale
        self.tracks_leave_trace = tracks_leave_trace
        self.pad_value = pad_value
        self.linewidth = linewidth
        self.fps = fps

    def visualize(
        self,
        video: torch.Tensor,  # (B,T,C,H,W), values in [0, 255]
        tracks: torch.Tensor,  # (B,T,N,2)
        visibility: torch.Tensor = None,  # (B,T,N,1)
        gt_tracks: torch.Tensor = None,
        segm_mask: torch.Tensor = None,
        filename: str = "video",
        writer=None,  # tensorboard SummaryWriter
        step: int = 0,
        query_frame: int = 0,
        save_video: bool = True,
        compensate_for_camera_motion: bool = False,
    ):
        """visualizer.py:87-135: the padded frames with every track drawn, (1, T - 1 + show_first_frame, 3, H + 2 pad,
        W + 2 pad) uint8 on the device; saved with :meth:`save_video` unless `save_video` is False."""
        self._check(segm_mask, gt_tracks, compensate_for_camera_motion)
        res_video = TV.render(video, tracks, visibility, mode=self.mode, linewidth=self.linewidth, pad_value=self.pad_value,
                              query_frame=query_frame, show_first_frame=self.show_first_frame)
        if save_video:
            self.save_video(res_video, filename=filename, writer=writer, step=step)
        return res_video

    def save_video(self, video, filename, writer=None, step=0):
        """visualizer.py:137-161: the video to a tensorboard `writer`, or frames [2:-1] of it (the reference's selection)
        to save_dir/filename.mp4 through imageio; without imageio this raises ImportError."""
        if writer is not None:
            writer.add_video(filename, video.to(torch.uint8), global_step=step, fps=self.fps)
            return
        try:
            import imageio
        except ImportError as e:
            raise ImportError("Visualizer.save_video needs imageio (with an mp4 backend) to encode the video; install "
                              "imageio[ffmpeg], pass a tensorboard writer, or call visualize(save_video=False) and write "
                              "the returned frames yourself") from e
        os.makedirs(self.save_dir, exist_ok=True)
        frames = video[0].permute(0, 2, 3, 1).cpu().numpy()
        save_path = os.path.join(self.save_dir, f"{filename}.mp4")
        video_writer = imageio.get_writer(save_path, fps=self.fps)
        for frame in frames[2:-1]:
            video_writer.append_data(frame)
        video_writer.close()
        print(f"Video saved to {save_path}")

    def draw_tracks_on_video(
        self,
        video: torch.Tensor,
        tracks: torch.Tensor,
        visibility: torch.Tensor = None,
        segm_mask: torch.Tensor = None,
        gt_tracks=None,
        query_frame: int = 0,
        compensate_for_camera_motion=False,
    ):
        """visualizer.py:163-295: as :meth:`visualize` on frames and tracks that are already padded (no pad_value)."""
        self._check(segm_mask, gt_tracks, compensate_for_camera_motion)
        return TV.render(video, tracks, visibility, mode=self.mode, linewidth=self.linewidth, pad_value=0,
                         query_frame=query_frame, show_first_frame=self.show_first_frame)

    def _check(self, segm_mask, gt_tracks, compensate_for_camera_motion):
        TV.check_options(mode=self.mode, grayscale=self.grayscale, tracks_leave_trace=self.tracks_leave_trace,
                         segm_mask=segm_mask, gt_tracks=gt_tracks, compensate_for_camera_motion=compensate_for_camera_motion)
