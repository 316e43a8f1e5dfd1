"""NumPy fp64 restatement of the per-joint heat-map moments (include/metro_hip.h, "per-joint heat-map covariance and peak
confidence"), for the tests: the softmax is oracle.forward.soft_argmax01's, the rest is the definition written out.

For one crop and head joint j, with p the softmax over the joint's S*S*D voxels and c = (x01, y01, z01) the voxel's fp32
linspace(0, 1, .) coordinates (exactly those the soft-argmax uses):  mu = sum p c,  Cov01 = sum p (c - mu)(c - mu)^T,
peak = max p."""
import numpy as np
import torch

from oracle.forward import soft_argmax01

COV6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))        # the kernels' order: xx, yy, zz, xy, xz, yz


def lin01(k):
    """tf.linspace(0, 1, k) as the soft-argmax evaluates it (fp32 step, fp32 product), as float64."""
    return (np.arange(k, dtype=np.float32) * (np.float32(1.0) / np.float32(k - 1))).astype(np.float64)


def moments(logits_nhwc, n_joints, depth):
    """logits [N, S, S, D*J] (channel d*J + j) -> (coords01 [N,J,3], cov01 [N,J,3,3], peak [N,J]) in fp64, and the oracle's own
    coords01 for the cross-check."""
    lg = torch.as_tensor(np.asarray(logits_nhwc, np.float64)).permute(0, 3, 1, 2)
    p, oracle_mu = soft_argmax01(lg, n_joints, depth)                  # p [N, J, H, W, D]
    p = p.numpy()
    side = p.shape[2]
    xs, zs = lin01(side), lin01(depth)
    c = np.stack(np.broadcast_arrays(xs[None, :, None], xs[:, None, None], zs[None, None, :]), -1)     # [H, W, D, 3]: (x<-W, y<-H, z<-D)
    mu = np.einsum('njhwd,hwdc->njc', p, c)
    dc = c[None, None] - mu[:, :, None, None, None, :]
    cov = np.einsum('njhwd,njhwda,njhwdb->njab', p, dc, dc)
    return mu, cov, p.max(axis=(2, 3, 4)), oracle_mu.numpy()


def cov6(cov):
    return np.stack([cov[..., a, b] for a, b in COV6], -1)


def metric_scale(spec):
    """s of Cov_mm = diag(s) Cov01 diag(s): the linear part of heatmap_to_metric (lrc of make_softargmax_args)."""
    last = spec.proc_side - 1
    lrc = last - (last % spec.stride) - 1
    return np.array([lrc * spec.box_size_mm / spec.proc_side, lrc * spec.box_size_mm / spec.proc_side, spec.box_size_mm])
