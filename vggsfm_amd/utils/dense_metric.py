"""How good a dense model is: the distances between a predicted cloud or mesh and a reference one, and the accuracy,
completeness (DTU) and precision, recall, F-score (Tanks and Temples) made of them.  The distances are vggsfm_amd.nearest's
(grid nearest point / nearest triangle, HIP) and every count and sum is vggn_distance_stats': exact integer counts, sums in
a fixed order, no torch.sum.  The reference has no namesake of anything here.

With d_p the distance of a `pred` point to the nearest point or face of `gt`, d_g that of a `gt` point to `pred`, both
searched within max_dist ("found" = there is one):

    accuracy, completeness                    the mean of the found d_p, of the found d_g  (nan when none is found)
    accuracy_rms, completeness_rms            the root of the mean of their squares
    accuracy_clamped, completeness_clamped    the means over ALL points, an unfound distance counted as max_dist
    overall, overall_rms, overall_clamped     (accuracy + completeness) / 2 of each kind
    num_pred, num_gt, found_pred, found_gt    exact integers
    thresholds, precision, recall, fscore     per threshold tau: P = #{d_p < tau} / num_pred, R = #{d_g < tau} / num_gt,
                                              F = 2 P R / (P + R), 0 when P + R = 0
"""
import math

import torch

from .. import nearest as NN


def metrics_from_stats(stats_pred, stats_gt, thresholds, max_dist):
    """The dictionary above from the two nearest.Stats (pred -> gt, gt -> pred): host arithmetic on a handful of numbers."""
    out = {"num_pred": int(stats_pred.num), "num_gt": int(stats_gt.num), "found_pred": int(stats_pred.found),
           "found_gt": int(stats_gt.found), "max_dist": float(max_dist), "thresholds": [float(t) for t in thresholds]}
    for name, s in (("accuracy", stats_pred), ("completeness", stats_gt)):
        out[name] = s.sum_d / s.found if s.found else math.nan
        out[name + "_rms"] = math.sqrt(s.sum_d2 / s.found) if s.found else math.nan
        out[name + "_clamped"] = (s.sum_d + (s.num - s.found) * float(max_dist)) / s.num if s.num else math.nan
    for kind in ("", "_rms", "_clamped"):
        out["overall" + kind] = (out["accuracy" + kind] + out["completeness" + kind]) / 2.0
    out["precision"] = [b / stats_pred.num if stats_pred.num else 0.0 for b in stats_pred.below]
    out["recall"] = [b / stats_gt.num if stats_gt.num else 0.0 for b in stats_gt.below]
    out["fscore"] = [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    return out


def _is_mesh(x):
    return hasattr(x, "_fields") and "faces" in x._fields


def _points(x):
    """the point set of a side: the vertices of a Mesh, the xyz of a FusedCloud, or the (N,3) tensor itself"""
    if _is_mesh(x):
        return x.vertices
    return x.xyz if hasattr(x, "_fields") and "xyz" in x._fields else x


def _distances(queries, target, max_dist, cell):
    """dist2 (M,) of the queries to `target`: to its faces when it is a Mesh, else to its points"""
    if _is_mesh(target):
        return NN.nearest_faces(target, queries, max_dist, cell).dist2
    return NN.nearest_points(_points(target), queries, max_dist, cell).dist2


def _evaluate(pred_points, pred, gt_points, gt, thresholds, max_dist, cell):
    thresholds = [float(t) for t in thresholds]
    stats_pred = NN.distance_stats(_distances(pred_points, gt, max_dist, cell), thresholds)
    stats_gt = NN.distance_stats(_distances(gt_points, pred, max_dist, cell), thresholds)
    return metrics_from_stats(stats_pred, stats_gt, thresholds, max_dist)


def cloud_to_cloud(pred, gt, thresholds, max_dist, cell=None):
    """pred (N,3), gt (M,3) device tensors (or FusedClouds) -> the metrics, point to nearest point in both directions."""
    pred, gt = _points(pred), _points(gt)
    return _evaluate(pred, pred, gt, gt, thresholds, max_dist, cell)


def cloud_to_mesh(pred_points, mesh, thresholds=(), max_dist=None, cell=None, return_distances=False):
    """pred_points (N,3) against a meshing.Mesh: d_p is the distance to the nearest FACE, d_g that of a mesh vertex to the
    nearest pred point.  max_dist is required.  return_distances: also the nearest.NearestFace of the points (face, distance,
    dist2, closest) as a second value."""
    if max_dist is None:
        raise ValueError("cloud_to_mesh needs max_dist")
    pred_points = _points(pred_points)
    out = _evaluate(pred_points, pred_points, mesh.vertices, mesh, thresholds, max_dist, cell)
    if return_distances:
        return out, NN.nearest_faces(mesh, pred_points, max_dist, cell, return_closest=True)
    return out


def evaluate_dense(pred, gt, thresholds, max_dist, transform=None, cell=None):
    """pred, gt: each a point set (N,3), a fusion.FusedCloud or a meshing.Mesh.  A mesh on either side is measured TO its
    faces in one direction and FROM its vertices in the other.  transform: (scale, R, t) of vggsfm_amd.sim3, applied to pred
    first (sim3.transform_points)."""
    if transform is not None:
        from .. import sim3

        scale, R, t = transform
        moved = sim3.transform_points(_points(pred).to(torch.float64), scale, R, t)
        pred = pred._replace(vertices=moved) if _is_mesh(pred) else moved
    return _evaluate(_points(pred), pred, _points(gt), gt, thresholds, max_dist, cell)
