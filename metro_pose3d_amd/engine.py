"""Host-side plumbing around libmetro_hip.so: plan creation, parameter folding/packing, device
buffers (torch) and the forward call.  No arithmetic of the hot path happens here: torch is used
for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.spec import ModelSpec

BN_EPS = 1e-5   # reference src/model/architectures.py:10

_NP_DTYPE = {_lib.METRO_F16: np.float16, _lib.METRO_F32: np.float32, _lib.METRO_F64: np.float64}
_PRECISIONS = {'f16': _lib.METRO_PREC_F16, 'f32': _lib.METRO_PREC_F32, 'f64': _lib.METRO_PREC_F64, 'f32m': _lib.METRO_PREC_F32M}


def _bn_scale_shift(params: Dict[str, np.ndarray], bn: str):
    g = params[bn + '/gamma'].astype(np.float64)
    b = params[bn + '/beta'].astype(np.float64)
    m = params[bn + '/moving_mean'].astype(np.float64)
    v = params[bn + '/moving_variance'].astype(np.float64)
    scale = g / np.sqrt(v + BN_EPS)
    return scale, b - m * scale


def pack_param(info: _lib.MetroParamInfo, params: Dict[str, np.ndarray]) -> np.ndarray:
    """One tensor of the plan's parameter blob, folded in fp64 and cast once.

    conv followed by BN (+ReLU):  w' = w * gamma/sqrt(var+eps) per c_out, b' = beta - mean*scale
    pre-activation BN (prologue): scale = gamma/sqrt(var+eps), shift = beta - mean*scale
    """
    conv = info.conv_var.decode()
    bn = info.bn_var.decode()
    dt = _NP_DTYPE[info.dtype]
    if info.kind == _lib.PARAM_CONV_W:
        w = params[conv + '/weights'].astype(np.float64)          # HWIO
        if w.shape != (info.kh, info.kw, info.c_in, info.c_out):
            raise ValueError(f'{conv}/weights has shape {w.shape}, plan expects '
                             f'{(info.kh, info.kw, info.c_in, info.c_out)}')
        if bn:
            w = w * _bn_scale_shift(params, bn)[0]
        packed = np.zeros((info.c_out, info.kh, info.kw_pad, info.c_in_pad), dtype=np.float64)
        packed[:, :, :info.kw, :info.c_in] = w.transpose(3, 0, 1, 2)
        return packed.astype(dt)
    if info.kind == _lib.PARAM_BIAS:
        v = _bn_scale_shift(params, bn)[1] if bn else params[conv + '/biases'].astype(np.float64)
    elif info.kind == _lib.PARAM_PRO_SCALE:
        v = _bn_scale_shift(params, bn)[0]
    elif info.kind == _lib.PARAM_PRO_SHIFT:
        v = _bn_scale_shift(params, bn)[1]
    else:
        raise ValueError(f'unknown parameter kind {info.kind}')
    if v.shape != (info.c_out,):
        raise ValueError(f'{info.name.decode()}: length {v.shape} != {info.c_out}')
    return v.astype(dt)


class Engine:
    """One plan on one GPU.  Not thread-safe (like the C plan it wraps)."""

    def __init__(self, spec: ModelSpec, params: Optional[Dict[str, np.ndarray]],
                 precision: str = 'f16', max_batch: int = 64, device: Optional[torch.device] = None):
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be 'f16', 'f32', 'f32m' or 'f64', got {precision!r}")
        self.lib = _lib.load()
        self.spec = spec
        self.precision = precision
        self.max_batch = int(max_batch)
        self._plan = C.c_void_p()
        cspec = spec.to_c(_PRECISIONS[precision])
        check(self.lib.metro_plan_create(C.byref(cspec), self.max_batch, C.byref(self._plan)),
              'metro_plan_create')
        self.cspec = cspec
        # hipGraph replay of the forward for batches <= METRO_HIPGRAPH_MAX_BATCH (default 0 = off:
        # measured on MI355X, batch 1..8 is bound by per-kernel dependency latency on the GPU, not by
        # host launches -- 0.661 ms eager vs 0.669 ms replayed, tools/graph_probe.py)
        import os
        gmax = int(os.environ.get('METRO_HIPGRAPH_MAX_BATCH', '0'))
        check(self.lib.metro_plan_set_graph_max_batch(self._plan, gmax), 'metro_plan_set_graph_max_batch')
        self.device = None
        self._blob = None
        self._ws = None
        self._u8_f32 = None
        self._moments = None
        self._heat = None
        self._modes = None
        self._prior = None
        self.heat_chunk = None       # crops per forward of a call with heat-map outputs (None: from HEAT_SCRATCH_CAP)
        if params is not None:
            if device is None:
                if not torch.cuda.is_available():
                    raise _lib.MetroError('no HIP device visible: the MeTRo hot path has no CPU fallback')
                device = torch.device('cuda', torch.cuda.current_device())
            self.bind(params, device)

    # ---- plan introspection (CPU-only safe) ---------------------------------------------
    def param_infos(self) -> List[_lib.MetroParamInfo]:
        out = []
        for i in range(self.lib.metro_plan_num_params(self._plan)):
            pi = _lib.MetroParamInfo()
            check(self.lib.metro_plan_param_info(self._plan, i, C.byref(pi)), 'metro_plan_param_info')
            out.append(pi)
        return out

    def layer_infos(self) -> List[_lib.MetroLayerInfo]:
        out = []
        for i in range(self.lib.metro_plan_num_layers(self._plan)):
            li = _lib.MetroLayerInfo()
            check(self.lib.metro_plan_layer_info(self._plan, i, C.byref(li)), 'metro_plan_layer_info')
            out.append(li)
        return out

    def layer_kernels(self, n: int) -> List[str]:
        """The kernel instantiation every layer runs on at batch n (metro_plan_layer_kernel: a dry run of the dispatch,
        no device needed).  The choice depends on the batch; tests/test_kernel_coverage.py holds every id to a test."""
        out = []
        buf = C.create_string_buffer(1024)
        for i in range(self.lib.metro_plan_num_layers(self._plan)):
            check(self.lib.metro_plan_layer_kernel(self._plan, i, int(n), buf, len(buf)), 'metro_plan_layer_kernel')
            out.append(buf.value.decode())
        return out

    @property
    def flops_per_image(self) -> float:
        return float(self.lib.metro_plan_flops_per_image(self._plan))

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.metro_plan_workspace_bytes(self._plan))

    @property
    def param_bytes(self) -> int:
        return int(self.lib.metro_plan_param_bytes(self._plan))

    def pack_params(self, params: Dict[str, np.ndarray]) -> np.ndarray:
        blob = np.zeros(self.param_bytes, dtype=np.uint8)
        for pi in self.param_infos():
            t = pack_param(pi, params)
            raw = np.ascontiguousarray(t).view(np.uint8).reshape(-1)
            if raw.size != pi.bytes:
                raise ValueError(f'{pi.name.decode()}: packed {raw.size} bytes, plan expects {pi.bytes}')
            blob[pi.offset:pi.offset + pi.bytes] = raw
        return blob

    # ---- device side -----------------------------------------------------------------------
    def bind(self, params: Dict[str, np.ndarray], device: torch.device) -> None:
        self.device = torch.device(device)
        blob = self.pack_params(params)
        with torch.cuda.device(self.device):
            self._blob = torch.from_numpy(blob).to(self.device)
            self._ws = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=self.device)
            if self._blob.data_ptr() % 256 or self._ws.data_ptr() % 256:
                raise _lib.MetroError('torch returned a device buffer that is not 256-byte aligned')
            check(self.lib.metro_plan_bind_params(self._plan, C.c_void_p(self._blob.data_ptr())),
                  'metro_plan_bind_params')

    def _check_images(self, images: torch.Tensor) -> torch.Tensor:
        s = self.spec.proc_side
        if self._blob is None:
            raise _lib.MetroError('Engine has no parameters bound')
        if not isinstance(images, torch.Tensor):
            raise ValueError('images must be a torch.Tensor on the GPU')
        if images.dim() != 4 or tuple(images.shape[1:]) != (s, s, 3):
            raise ValueError(f'images must be [N,{s},{s},3] NHWC, got {tuple(images.shape)}')
        if images.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f'images must be float32 in [0,1] or uint8 (byte b = b / 255), got {images.dtype}')
        if images.device != self.device:
            raise ValueError(f'images are on {images.device}, the plan is on {self.device}')
        if images.shape[0] < 1 or images.shape[0] > self.max_batch:
            raise ValueError(f'batch {images.shape[0]} outside [1, {self.max_batch}]')
        images = images.contiguous()
        if images.dtype == torch.uint8 and images.data_ptr() % 16:
            images = images.clone()         # metro_forward_u8 fetches 16-byte pieces: a misaligned view is copied once
        return images

    def _as_float32(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 crops -> the fp32 image they stand for (metro_images_u8_to_f32: byte / 255, an IEEE divide), in a buffer the
        engine owns (allocated on first use, max_batch crops): what the parity precisions, whose forward takes fp32, run on."""
        n, s = images.shape[0], self.spec.proc_side
        if self._u8_f32 is None:
            self._u8_f32 = torch.empty((self.max_batch, s, s, 3), dtype=torch.float32, device=self.device)
        out = self._u8_f32[:n]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.metro_images_u8_to_f32(C.c_void_p(images.data_ptr()), images.numel(), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(stream)), 'metro_images_u8_to_f32')
        return out

    def heat_shapes(self, n: int):
        """Shapes of the heat-map marginals of n crops: xy (n, Jout, S, S) and z (n, Jout, D)."""
        s, j = self.spec.heatmap_side, self.spec.skeleton.n_out
        return (n, j, s, s), (n, j, self.spec.depth)

    def _heat_chunk(self) -> int:
        """Crops per bound forward: `heat_chunk` if set, else as many as keep the scratch within HEAT_SCRATCH_CAP bytes."""
        if self.heat_chunk is not None:
            return max(1, min(int(self.heat_chunk), self.max_batch))
        k = self.max_batch
        while k > 1 and int(self.lib.metro_plan_heatmaps_scratch_bytes(self._plan, k)) > self.HEAT_SCRATCH_CAP:
            k = (k + 1) // 2
        return k

    def _forward_heat(self, images, out, coords01, cov01, peak, heat_xy, heat_z) -> torch.Tensor:
        """forward() with heat-map buffers: binds them to the plan chunk by chunk (host state, read at enqueue), runs the plain
        forward on each chunk and unbinds.  The status words of every chunk are put back so that status_words(n) is the call's."""
        n, k = images.shape[0], self._heat_chunk()
        nb = int(self.lib.metro_plan_heatmaps_scratch_bytes(self._plan, k))
        if self._heat is None or self._heat.numel() < nb:
            self._heat = torch.empty(nb, dtype=torch.uint8, device=self.device)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        words = []
        try:
            for i in range(0, n, k):
                m = min(k, n - i)
                check(self.lib.metro_plan_bind_heatmaps(self._plan, C.c_void_p(heat_xy[i:i + m].data_ptr()),
                                                        C.c_void_p(heat_z[i:i + m].data_ptr()), C.c_void_p(self._heat.data_ptr()), k),
                      'metro_plan_bind_heatmaps')
                self.forward(images[i:i + m], out[i:i + m], part(coords01, i, m), part(cov01, i, m), part(peak, i, m))
                if n > k:
                    words.append(self.status_words(m).clone())
        finally:
            check(self.lib.metro_plan_bind_heatmaps(self._plan, None, None, None, 0), 'metro_plan_bind_heatmaps')
        if words:
            self.status_words(n).copy_(torch.cat(words))
        return out

    HEAT_SCRATCH_CAP = 1 << 30

    MODE_STATS = 11          # mass, peak, coords01 (x, y, z), cov01 (xx, yy, zz, xy, xz, yz)

    def forward_modes(self, images: torch.Tensor, k: int = 2, radius: int = 1, out: Optional[torch.Tensor] = None,
                      coords01: Optional[torch.Tensor] = None, cov01: Optional[torch.Tensor] = None,
                      peak: Optional[torch.Tensor] = None, heat_xy: Optional[torch.Tensor] = None,
                      heat_z: Optional[torch.Tensor] = None):
        """forward() that also returns every output joint's heat-map modes -> (poses, voxel int32 [n, Jout, k], stats fp32
        [n, Jout, k, 11]): the k places the joint may be (local maxima of its logits, none within 2 * radius voxels of another
        in every axis, by decreasing logit), `voxel` their linear index (y * S + x) * D + d or -1 for a missing mode, `stats`
        per mode the mass, peak, coords01 (x, y, z) and cov01 (xx, yy, zz, xy, xz, yz) of the joint's softmax over the window
        of `radius` voxels around it (metro_plan_bind_modes, include/metro_hip.h, holds the definition).  Binds the two
        outputs to the plan chunk by chunk (host state, read at enqueue), calls forward() with the other arguments and
        unbinds; every other output keeps the bits forward() gives it.  The engine owns the scratch; the call is made of
        several forwards by the rule of the heat-map outputs (HEAT_SCRATCH_CAP, heat_chunk)."""
        images = self._check_images(images)
        n, nj = images.shape[0], self.spec.skeleton.n_out
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.METRO_MAX_MODES:
            raise ValueError(f'k must be an int in [1, {_lib.METRO_MAX_MODES}], got {k!r}')
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= _lib.METRO_MAX_MODE_RADIUS:
            raise ValueError(f'radius must be an int in [0, {_lib.METRO_MAX_MODE_RADIUS}], got {radius!r}')
        if out is None:
            out = torch.empty((n, nj, 3), dtype=torch.float32, device=self.device)
        else:
            self._check_out('out', out, (n, nj, 3))
        voxel = torch.empty((n, nj, k), dtype=torch.int32, device=self.device)
        stats = torch.empty((n, nj, k, self.MODE_STATS), dtype=torch.float32, device=self.device)
        step = self._heat_chunk()
        nb = int(self.lib.metro_plan_modes_scratch_bytes(self._plan, step))
        if self._modes is None or self._modes.numel() < nb:
            self._modes = torch.empty(nb, dtype=torch.uint8, device=self.device)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        words = []
        try:
            for i in range(0, n, step):
                m = min(step, n - i)
                check(self.lib.metro_plan_bind_modes(self._plan, C.c_void_p(voxel[i:i + m].data_ptr()),
                                                     C.c_void_p(stats[i:i + m].data_ptr()), C.c_void_p(self._modes.data_ptr()),
                                                     step, k, radius), 'metro_plan_bind_modes')
                self.forward(images[i:i + m], out[i:i + m], part(coords01, i, m), part(cov01, i, m), part(peak, i, m),
                             part(heat_xy, i, m), part(heat_z, i, m))
                if n > step:
                    words.append(self.status_words(m).clone())
        finally:
            check(self.lib.metro_plan_bind_modes(self._plan, None, None, None, 0, 0, 0), 'metro_plan_bind_modes')
        if words:
            self.status_words(n).copy_(torch.cat(words))
        return out, voxel, stats

    POST_STATS = 11          # log_evidence, peak', coords01' (x, y, z), cov01' (xx, yy, zz, xy, xz, yz)
    PRIOR_WORDS = 9          # mu (x, y, z), precision (xx, yy, zz, xy, xz, yz), in coords01 units

    def forward_posterior(self, images: torch.Tensor, prior: torch.Tensor, out: Optional[torch.Tensor] = None,
                          coords01: Optional[torch.Tensor] = None, cov01: Optional[torch.Tensor] = None,
                          peak: Optional[torch.Tensor] = None, heat_xy: Optional[torch.Tensor] = None,
                          heat_z: Optional[torch.Tensor] = None):
        """forward() that also returns every output joint's heat-map posterior under a Gaussian prior -> (poses, post fp32
        [n, Jout, 11]).  `prior` fp32 [n, Jout, 9] on the plan's device, output joint order: per joint mu (x, y, z in coords01
        units) and the precision (xx, yy, zz, xy, xz, yz; positive semi-definite, may be singular, all zero: no knowledge).
        `post` per joint: log_evidence, and the peak, coords01 (x, y, z) and cov01 (xx, yy, zz, xy, xz, yz) of the joint's
        softmax times the prior, over the whole volume (metro_plan_bind_prior, include/metro_hip.h, holds the definition).
        Binds prior and output to the plan chunk by chunk (host state, read at enqueue), calls forward() with the other
        arguments and unbinds; every other output keeps the bits forward() gives it.  The engine owns the scratch; the call is
        made of several forwards by the rule of the heat-map outputs (HEAT_SCRATCH_CAP, heat_chunk)."""
        images = self._check_images(images)
        n, nj = images.shape[0], self.spec.skeleton.n_out
        if not isinstance(prior, torch.Tensor) or prior.dtype != torch.float32 or tuple(prior.shape) != (n, nj, self.PRIOR_WORDS):
            raise ValueError(f'prior must be a float32 tensor [{n}, {nj}, {self.PRIOR_WORDS}] (mu x, y, z; precision xx, yy, zz, xy, '
                             f'xz, yz), got {tuple(prior.shape) if isinstance(prior, torch.Tensor) else type(prior)}'
                             f'{" of " + str(prior.dtype) if isinstance(prior, torch.Tensor) else ""}')
        if prior.device != self.device:
            raise ValueError(f'prior is on {prior.device}, the plan is on {self.device}')
        prior = prior.contiguous()
        if out is None:
            out = torch.empty((n, nj, 3), dtype=torch.float32, device=self.device)
        else:
            self._check_out('out', out, (n, nj, 3))
        post = torch.empty((n, nj, self.POST_STATS), dtype=torch.float32, device=self.device)
        step = self._heat_chunk()
        nb = int(self.lib.metro_plan_prior_scratch_bytes(self._plan, step))
        if self._prior is None or self._prior.numel() < nb:
            self._prior = torch.empty(nb, dtype=torch.uint8, device=self.device)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        words = []
        try:
            for i in range(0, n, step):
                m = min(step, n - i)
                check(self.lib.metro_plan_bind_prior(self._plan, C.c_void_p(prior[i:i + m].data_ptr()),
                                                     C.c_void_p(post[i:i + m].data_ptr()), C.c_void_p(self._prior.data_ptr()), step),
                      'metro_plan_bind_prior')
                self.forward(images[i:i + m], out[i:i + m], part(coords01, i, m), part(cov01, i, m), part(peak, i, m),
                             part(heat_xy, i, m), part(heat_z, i, m))
                if n > step:
                    words.append(self.status_words(m).clone())
        finally:
            check(self.lib.metro_plan_bind_prior(self._plan, None, None, None, 0), 'metro_plan_bind_prior')
        if words:
            self.status_words(n).copy_(torch.cat(words))
        return out, post

    def forward_track_posterior(self, images: torch.Tensor, state: torch.Tensor, slot: torch.Tensor, times: torch.Tensor,
                                records: torch.Tensor, mirror: torch.Tensor, coords: str, depth: str = 'none',
                                accel_psd: float = 4e6, max_age_s: float = 1.0, near_mm: float = 100.0,
                                sigma_floor_mm: float = 30.0, cov_scale: float = 1.0, out: Optional[torch.Tensor] = None,
                                coords01: Optional[torch.Tensor] = None, cov01: Optional[torch.Tensor] = None,
                                peak: Optional[torch.Tensor] = None, heat_xy: Optional[torch.Tensor] = None,
                                heat_z: Optional[torch.Tensor] = None):
        """forward_posterior() whose prior rows the forward writes itself, from a track table -> (poses, post fp32 [n, Jout, 11],
        prior fp32 [n, Jout, 9], reason int32 [n, Jout]).  All on the plan's device, contiguous, read when the forward runs:
        state float64 [T, Jout, 28], the constant-velocity table of the follow calls (frames.TrackTable.state), 1 <= T <= 128;
        slot int32 [n], the table slot of every crop (-1 or outside the table: no prior); times float64 [n], the crops' exposure
        times in seconds on the clock of the table; records uint8 [n, 208], the crops' MetroPlacement records
        (frames.pack_placements, or what the view expansion wrote); mirror int32 [Jout], the output-order mirror joints.
        coords 'camera' or 'world': the frame the table lives in.  depth, accel_psd, max_age_s, near_mm, sigma_floor_mm and
        cov_scale: heads.track_prior_params, which holds their meaning and says of the defaults that they are design choices,
        not measurements.  Per crop and output joint the track's state is advanced to the crop's time, projected through the
        crop's virtual camera and written as the prior row `prior` (nine zeros and a reason word other than 0 where the track
        gives none: `post` is then the plain distribution's, log_evidence exactly 0); `post` is forward_posterior's under
        those rows (metro_plan_bind_track_prior, include/metro_hip.h, holds the definition).  Binds chunk by chunk by the rule
        of forward_posterior and unbinds; every other output keeps the bits forward() gives it.  depth='root' reads the
        forward's own coords01: one is allocated when none is passed."""
        from metro_pose3d_amd.heads import ASSOC_MAX, TRACK_STATE_DOUBLES, track_prior_params
        images = self._check_images(images)
        n, nj = images.shape[0], self.spec.skeleton.n_out
        params = track_prior_params(coords, depth, accel_psd, max_age_s, near_mm, sigma_floor_mm, cov_scale)
        rec_bytes = C.sizeof(_lib.MetroPlacement)

        def given(name, t, dtype, shape, what):
            if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError(f'{name} must be a contiguous {str(dtype).replace("torch.", "")} {list(shape)} tensor on {self.device} '
                                 f'({what}), got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        if not isinstance(state, torch.Tensor) or state.dim() != 3 or not 1 <= state.shape[0] <= ASSOC_MAX:
            raise ValueError(f'state must be a float64 tensor [T, {nj}, {TRACK_STATE_DOUBLES}] with 1 <= T <= {ASSOC_MAX} '
                             f'(frames.TrackTable.state), got {tuple(getattr(state, "shape", ()))}')
        given('state', state, torch.float64, (state.shape[0], nj, TRACK_STATE_DOUBLES), 'frames.TrackTable.state')
        given('slot', slot, torch.int32, (n,), 'the table slot of every crop')
        given('times', times, torch.float64, (n,), 'the exposure time of every crop, seconds')
        given('records', records, torch.uint8, (n, rec_bytes), 'the MetroPlacement record of every crop')
        given('mirror', mirror, torch.int32, (nj,), 'the output-order mirror joints')
        if records.data_ptr() % 4:
            records = records.clone()
        if out is None:
            out = torch.empty((n, nj, 3), dtype=torch.float32, device=self.device)
        else:
            self._check_out('out', out, (n, nj, 3))
        if depth == 'root' and coords01 is None:
            coords01 = torch.empty((n, self.spec.skeleton.n_head, 3), dtype=torch.float32, device=self.device)
        post = torch.empty((n, nj, self.POST_STATS), dtype=torch.float32, device=self.device)
        prior = torch.empty((n, nj, self.PRIOR_WORDS), dtype=torch.float32, device=self.device)
        reason = torch.empty((n, nj), dtype=torch.int32, device=self.device)
        step = self._heat_chunk()
        nb = int(self.lib.metro_plan_prior_scratch_bytes(self._plan, step))
        if self._prior is None or self._prior.numel() < nb:
            self._prior = torch.empty(nb, dtype=torch.uint8, device=self.device)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        words = []
        try:
            for i in range(0, n, step):
                m = min(step, n - i)
                check(self.lib.metro_plan_bind_track_prior(self._plan, ptr(state), int(state.shape[0]), ptr(slot[i:i + m]),
                                                           ptr(times[i:i + m]), ptr(records[i:i + m]), ptr(mirror), C.byref(params),
                                                           ptr(prior[i:i + m]), ptr(reason[i:i + m]), ptr(post[i:i + m]),
                                                           ptr(self._prior), step), 'metro_plan_bind_track_prior')
                self.forward(images[i:i + m], out[i:i + m], part(coords01, i, m), part(cov01, i, m), part(peak, i, m),
                             part(heat_xy, i, m), part(heat_z, i, m))
                if n > step:
                    words.append(self.status_words(m).clone())
        finally:
            check(self.lib.metro_plan_bind_track_prior(self._plan, None, 0, None, None, None, None, None, None, None, None, None, 0),
                  'metro_plan_bind_track_prior')
        if words:
            self.status_words(n).copy_(torch.cat(words))
        return out, post, prior, reason

    def forward_view_fusion(self, images: torch.Tensor, places: torch.Tensor, rows: torch.Tensor, starts: torch.Tensor,
                            n_persons: int, mirror: torch.Tensor, fusion, weights: str = 'covariance', min_angle_deg: float = 2.0,
                            centres: Optional[torch.Tensor] = None, n_views: int = 1, out: Optional[torch.Tensor] = None,
                            coords01: Optional[torch.Tensor] = None, cov01: Optional[torch.Tensor] = None,
                            peak: Optional[torch.Tensor] = None, heat_xy: Optional[torch.Tensor] = None,
                            heat_z: Optional[torch.Tensor] = None):
        """forward() whose heat-map marginals are fused over the cameras of every person, on a grid of world points ->
        (poses, coords01, fused points fp32 [P, Jout, 3] world mm, cov fp32 [P, Jout, 9] mm^2, stats fp32 [P, Jout, 2]: the
        largest weight and the agreement, info int32 [P, Jout, 2]: rows used and edge, centres fp32 [P, Jout, 3]).  All on the
        plan's device, contiguous, read when the forward runs: places uint8 [n, 208], the crops' MetroPlacement records; rows
        int32 [R] and starts int32 [n_persons + 1], the CSR heads.triangulate_joints reads (frames.person_groups); mirror int32
        [Jout], the output-order mirror joints; fusion: heads.fusion_params(...), which holds the keywords' meaning and says of
        the defaults that they are design choices; n_views: the rows per camera, a row counts 1 / n_views.
        centres None: the cube of every joint is centred on its triangulated point -- heads.triangulate_joints' launch on this
        forward's coords01 (and cov01 with weights 'covariance', allocated here when not passed), with `weights` and
        `min_angle_deg`; `centres` is that launch's points bit for bit.  centres fp32 [P, Jout, 3] (a track's prediction, say):
        used as they are, returned as a copy.  metro_plan_bind_view_fusion (include/metro_hip.h) holds the definition.
        Binds the heat-maps (heat_xy, heat_z: allocated when not passed) and the fusion together and unbinds after the enqueue;
        every other output keeps the bits forward() gives it.  A person's rows must share one forward: ValueError where the
        call would be split (n above the chunk of bound forwards, `heat_chunk`)."""
        images = self._check_images(images)
        n, sk = images.shape[0], self.spec.skeleton
        nj = sk.n_out
        params = fusion.record(weights, min_angle_deg, n_views)
        step = self._heat_chunk()
        if n > step:
            raise ValueError(f'{n} crops would be split into forwards of {step} (heat_chunk): a person\'s rows must share one forward')
        if isinstance(n_persons, (bool, np.bool_)) or not isinstance(n_persons, (int, np.integer)) or n_persons < 0:
            raise ValueError(f'n_persons must be an integer >= 0, got {n_persons!r}')
        n_persons = int(n_persons)
        rec_bytes = C.sizeof(_lib.MetroPlacement)

        def given(name, t, dtype, shape, what):
            if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError(f'{name} must be a contiguous {str(dtype).replace("torch.", "")} {list(shape)} tensor on {self.device} '
                                 f'({what}), got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        given('places', places, torch.uint8, (n, rec_bytes), 'the MetroPlacement record of every crop')
        if not isinstance(rows, torch.Tensor) or rows.dim() != 1:
            raise ValueError(f'rows must be an int32 tensor [R] (frames.person_groups), got {tuple(getattr(rows, "shape", ()))}')
        given('rows', rows, torch.int32, (rows.numel(),), 'the crop rows of the persons')
        given('starts', starts, torch.int32, (n_persons + 1,), 'the first row of every person, and the end')
        given('mirror', mirror, torch.int32, (nj,), 'the output-order mirror joints')
        if centres is not None:
            given('centres', centres, torch.float32, (n_persons, nj, 3), 'the centre of the cube of every joint, world mm')
        if places.data_ptr() % 4:
            places = places.clone()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        if out is None:
            out = f32(n, nj, 3)
        else:
            self._check_out('out', out, (n, nj, 3))
        if coords01 is None:
            coords01 = f32(n, sk.n_head, 3)
        if centres is None and weights == 'covariance' and cov01 is None and peak is None:
            cov01, peak = f32(n, sk.n_head, 6), f32(n, sk.n_head)
        if (heat_xy is None) != (heat_z is None):
            raise ValueError('heat_xy and heat_z go together: pass both or neither')
        if heat_xy is None:
            heat_xy, heat_z = (f32(*s) for s in self.heat_shapes(n))
        points, cov, stats, centres_out = f32(n_persons, nj, 3), f32(n_persons, nj, 9), f32(n_persons, nj, 2), f32(n_persons, nj, 3)
        info = torch.empty((n_persons, nj, 2), dtype=torch.int32, device=self.device)
        # an empty tensor has no address: any aligned one stands for it, nothing is read or written through it
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else self._ws.data_ptr())
        try:
            check(self.lib.metro_plan_bind_view_fusion(self._plan, ptr(heat_xy), ptr(places), ptr(rows), int(rows.numel()), ptr(starts),
                                                       n_persons, ptr(mirror), ptr(centres) if centres is not None else None,
                                                       C.byref(params), ptr(points), ptr(cov), ptr(stats), ptr(info), ptr(centres_out),
                                                       step), 'metro_plan_bind_view_fusion')
            self.forward(images, out, coords01, cov01, peak, heat_xy, heat_z)
        finally:
            check(self.lib.metro_plan_bind_view_fusion(self._plan, None, None, None, 0, None, 0, None, None, None, None, None, None, None,
                                                       None, 0), 'metro_plan_bind_view_fusion')
        return out, coords01, points, cov, stats, info, centres_out

    def forward_skeleton_modes(self, images: torch.Tensor, lengths: torch.Tensor, k: int = 2, radius: int = 1, edges=None,
                               sigma_mm: float = 20.0, sigma_rel: float = 0.0, cov_scale: float = 1.0, min_length_mm: float = 1.0,
                               out: Optional[torch.Tensor] = None, coords01: Optional[torch.Tensor] = None,
                               cov01: Optional[torch.Tensor] = None, peak: Optional[torch.Tensor] = None,
                               heat_xy: Optional[torch.Tensor] = None, heat_z: Optional[torch.Tensor] = None):
        """forward_modes() whose modes are chosen among by the person's bone lengths -> (poses, voxel int32 [n, Jout, k], stats
        fp32 [n, Jout, k, 11], choice int32 [n, Jout]: the mode of every joint in the most probable assignment of the whole
        skeleton (-1: a joint without a usable mode), prob fp32 [n, Jout, k]: the marginal of every mode, info fp32 [n, Jout, 2]:
        (log_evidence, log_map) of the joint's component, coords01_sel fp32 [n, J_head, 3]: coords01 with the chosen modes'
        means in place of the plain ones).  lengths: float64 [n, E] in mm on the plan's device, contiguous, read when the forward
        runs (Follower.bone_lengths_for's tensor as it is); NaN or <= 0: that bone is unknown for that crop.  edges: [E, 2]
        output-joint indices, a forest (default: the skeleton's own edges).  The likelihood of a pair of modes on a bone is a
        Gaussian of the distance between their means in heatmap_to_metric's scale (heads.skeleton_mode_params holds the
        keywords' meaning and says of the defaults that they are design choices; metro_plan_bind_skeleton_modes,
        include/metro_hip.h, holds the definition).  Binds the modes and the skeleton together, chunk by chunk, and unbinds
        after the enqueue; every other output keeps the bits forward_modes() gives it."""
        from metro_pose3d_amd.heads import skeleton_edges, skeleton_mode_params
        from metro_pose3d_amd.inference import _metric_map
        images = self._check_images(images)
        n, sk = images.shape[0], self.spec.skeleton
        nj = sk.n_out
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.METRO_MAX_MODES:
            raise ValueError(f'k must be an int in [1, {_lib.METRO_MAX_MODES}], got {k!r}')
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= _lib.METRO_MAX_MODE_RADIUS:
            raise ValueError(f'radius must be an int in [0, {_lib.METRO_MAX_MODE_RADIUS}], got {radius!r}')
        e = skeleton_edges(sk.edges_array() if edges is None else edges, nj)
        ne = len(e)
        params = skeleton_mode_params(_metric_map(self.spec)[0], sigma_mm, sigma_rel, cov_scale, min_length_mm)
        if (not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.float64 or tuple(lengths.shape) != (n, ne)
                or lengths.device != self.device or not lengths.is_contiguous()):
            raise ValueError(f'lengths must be a contiguous float64 [{n}, {ne}] tensor on {self.device} (mm, one row per crop), got '
                             f'{getattr(lengths, "dtype", type(lengths))} {tuple(getattr(lengths, "shape", ()))}')
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        if out is None:
            out = f32(n, nj, 3)
        else:
            self._check_out('out', out, (n, nj, 3))
        if coords01 is None:
            coords01 = f32(n, sk.n_head, 3)
        voxel = torch.empty((n, nj, k), dtype=torch.int32, device=self.device)
        stats = f32(n, nj, k, self.MODE_STATS)
        choice = torch.empty((n, nj), dtype=torch.int32, device=self.device)
        prob, info, sel = f32(n, nj, k), f32(n, nj, 2), f32(n, sk.n_head, 3)
        step = self._heat_chunk()
        nb = int(self.lib.metro_plan_modes_scratch_bytes(self._plan, step))
        if self._modes is None or self._modes.numel() < nb:
            self._modes = torch.empty(nb, dtype=torch.uint8, device=self.device)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        # an empty tensor has no address: any aligned one stands for it, nothing is read or written through it
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else self._ws.data_ptr())
        words = []
        try:
            for i in range(0, n, step):
                m = min(step, n - i)
                check(self.lib.metro_plan_bind_modes(self._plan, ptr(voxel[i:i + m]), ptr(stats[i:i + m]), C.c_void_p(self._modes.data_ptr()),
                                                     step, k, radius), 'metro_plan_bind_modes')
                check(self.lib.metro_plan_bind_skeleton_modes(self._plan, ptr(voxel[i:i + m]), ptr(stats[i:i + m]), k, ptr(lengths[i:i + m]),
                                                              e.ctypes.data_as(C.c_void_p) if ne else None, ne, C.byref(params),
                                                              ptr(prob[i:i + m]), ptr(choice[i:i + m]), ptr(info[i:i + m]),
                                                              ptr(sel[i:i + m]), step), 'metro_plan_bind_skeleton_modes')
                self.forward(images[i:i + m], out[i:i + m], coords01[i:i + m], part(cov01, i, m), part(peak, i, m),
                             part(heat_xy, i, m), part(heat_z, i, m))
                if n > step:
                    words.append(self.status_words(m).clone())
        finally:
            check(self.lib.metro_plan_bind_skeleton_modes(self._plan, None, None, 0, None, None, 0, None, None, None, None, None, 0),
                  'metro_plan_bind_skeleton_modes')
            check(self.lib.metro_plan_bind_modes(self._plan, None, None, None, 0, 0, 0), 'metro_plan_bind_modes')
        if words:
            self.status_words(n).copy_(torch.cat(words))
        return out, voxel, stats, choice, prob, info, sel

    def forward(self, images: torch.Tensor, out: Optional[torch.Tensor] = None,
                coords01: Optional[torch.Tensor] = None, cov01: Optional[torch.Tensor] = None,
                peak: Optional[torch.Tensor] = None, heat_xy: Optional[torch.Tensor] = None,
                heat_z: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images fp32 [n,256,256,3] on the plan's device -> poses fp32 [n,Jout,3] (mm).  Enqueued
        on torch's current stream; no synchronisation.  `coords01`: an fp32 [n, J_head, 3] device tensor that also receives
        the soft-argmax coordinates in [0,1] (head order; metro_forward_coords01: the same poses, from the same launches).
        uint8 images (byte b = the fp32 value b / 255) give the bits of the fp32 call on those values: precision 'f16' reads
        the bytes in its first kernel (metro_forward_u8), the others expand them once (metro_images_u8_to_f32).
        `cov01` / `peak` (together): fp32 [n, J_head, 6] and [n, J_head] device tensors that receive every joint's heat-map
        covariance (xx, yy, zz, xy, xz, yz in the units of coords01) and peak probability, head order -- the spread of the
        joint's own softmax distribution in the crop's virtual-camera axes, not of the root-relative pose
        (metro_forward_moments: the same launch count, the same poses and coords01).  With both None the call goes to the
        entries it always went to.
        `heat_xy` / `heat_z` (together): fp32 [n, Jout, S, S] and [n, Jout, D] device tensors (heat_shapes) that receive every
        output joint's heat-map marginals, xy[i, r, y, x] = sum_d p and z[i, r, d] = sum_{y,x} p of its softmax volume
        (metro_plan_bind_heatmaps: the same entries write them from the logits of the same forward; every other output keeps
        its bits).  The engine owns the scratch (the one-launch head's fp32 logits: S * S * D * J_head * 4 bytes a crop).  Only
        where that would pass HEAT_SCRATCH_CAP for max_batch crops -- or where `heat_chunk` is set -- the call is made of
        forwards of at most that many crops each; the kernels a forward dispatches follow its batch, so all outputs are then
        those of Engine.forward on those chunks, which need not be the bits of one forward of all n crops."""
        images = self._check_images(images)
        n = images.shape[0]
        if (cov01 is None) != (peak is None):
            raise ValueError('cov01 and peak go together: pass both or neither')
        if (heat_xy is None) != (heat_z is None):
            raise ValueError('heat_xy and heat_z go together: pass both or neither')
        if cov01 is not None:
            self._check_out('cov01', cov01, (n, self.spec.skeleton.n_head, 6))
            self._check_out('peak', peak, (n, self.spec.skeleton.n_head))
        if heat_xy is not None:
            self._check_out('heat_xy', heat_xy, self.heat_shapes(n)[0])
            self._check_out('heat_z', heat_z, self.heat_shapes(n)[1])
        if out is None:
            out = torch.empty((n, self.spec.skeleton.n_out, 3), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if coords01 is not None:
            self._check_coords01(coords01, n)
        if heat_xy is not None:
            return self._forward_heat(images, out, coords01, cov01, peak, heat_xy, heat_z)
        if cov01 is not None:
            u8 = images.dtype == torch.uint8 and self.precision == 'f16'
            if images.dtype == torch.uint8 and not u8:
                images = self._as_float32(images)
            if self._moments is None:
                nb = int(self.lib.metro_moments_scratch_bytes(C.byref(self.cspec), self.max_batch))
                self._moments = torch.empty(nb, dtype=torch.uint8, device=self.device)
            check(self.lib.metro_forward_moments(self._plan, C.c_void_p(images.data_ptr()), int(u8), n, C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(coords01.data_ptr() if coords01 is not None else 0),
                                                 C.c_void_p(cov01.data_ptr()), C.c_void_p(peak.data_ptr()),
                                                 C.c_void_p(self._moments.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                                 C.c_void_p(stream)), 'metro_forward_moments')
            return out
        if images.dtype == torch.uint8:
            if self.precision == 'f16':
                check(self.lib.metro_forward_u8(self._plan, C.c_void_p(images.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(coords01.data_ptr() if coords01 is not None else 0),
                                                C.c_void_p(self._ws.data_ptr()), C.c_void_p(stream)), 'metro_forward_u8')
                return out
            images = self._as_float32(images)
        if coords01 is None:
            check(self.lib.metro_forward(self._plan, C.c_void_p(images.data_ptr()), n,
                                         C.c_void_p(out.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                         C.c_void_p(stream)), 'metro_forward')
            return out
        check(self.lib.metro_forward_coords01(self._plan, C.c_void_p(images.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(coords01.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                              C.c_void_p(stream)), 'metro_forward_coords01')
        return out

    def _check_coords01(self, coords01, n: int) -> None:
        shape = (n, self.spec.skeleton.n_head, 3)
        if (not isinstance(coords01, torch.Tensor) or coords01.dtype != torch.float32 or tuple(coords01.shape) != shape
                or coords01.device != self.device or not coords01.is_contiguous()):
            raise ValueError(f'coords01 must be a contiguous float32 {list(shape)} tensor on {self.device}, got '
                             f'{getattr(coords01, "dtype", type(coords01))} {tuple(getattr(coords01, "shape", ()))}')

    def _check_out(self, name: str, t, shape) -> None:
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape)
                or t.device != self.device or not t.is_contiguous()):
            raise ValueError(f'{name} must be a contiguous float32 {list(shape)} tensor on {self.device}, got '
                             f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')

    def check_finite(self, n: int) -> None:
        """Non-finite screen of the last forward(n) on this engine: raises _lib.NonFiniteError when activations overflowed
        the arithmetic mode on their way to the soft-argmax (metro_forward_status).  Synchronises the current stream."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        bad = C.c_int32(0)
        check(self.lib.metro_forward_status(self._plan, C.c_void_p(self._ws.data_ptr()), int(n), C.c_void_p(stream), C.byref(bad)),
              f'{self.spec.arch_name} stride {self.spec.stride} in precision {self.precision!r}')

    def status_words(self, n: int) -> torch.Tensor:
        """Device view (int32 [n]) of the non-finite words the LAST forward(n) on this engine wrote (1 = that crop reached the
        soft-argmax with non-finite statistics).  No synchronisation: valid until the next forward, on the same stream."""
        off = int(self.lib.metro_plan_status_offset(self._plan))
        return self._ws[off:off + 4 * int(n)].view(torch.int32)

    def forward_upto(self, images: torch.Tensor, layer: int, second: bool = False) -> torch.Tensor:
        """Runs layers [0..layer] and returns that layer's output tensor [n,h,w,c] (a copy); `second` selects
        the second output of a fused launch (MetroLayerInfo.out2_offset)."""
        images = self._check_images(images)
        if images.dtype == torch.uint8:      # layer dumps and timings take the fp32 image the bytes stand for
            images = self._as_float32(images)
        n = images.shape[0]
        li = self.layer_infos()[layer]
        poses = torch.empty((n, self.spec.skeleton.n_out, 3), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.metro_forward_upto(self._plan, C.c_void_p(images.data_ptr()), n,
                                          C.c_void_p(poses.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                          C.c_void_p(stream), layer), 'metro_forward_upto')
        if li.kind == _lib.LAYER_SOFTARGMAX:
            return poses
        dt = {_lib.METRO_F16: torch.float16, _lib.METRO_F32: torch.float32,
              _lib.METRO_F64: torch.float64}[li.out_dtype]
        if second:
            if li.out2_offset < 0:
                raise ValueError(f'{li.name.decode()}: layer has no second output')
            nb2 = li.h_out * li.w_out * li.out2_channels * 2 * n
            return self._ws[li.out2_offset:li.out2_offset + nb2].view(torch.float16).view(
                n, li.h_out, li.w_out, li.out2_channels).clone()
        nbytes = li.out_bytes_per_image * n
        raw = self._ws[li.out_offset:li.out_offset + nbytes]
        return raw.view(dt).view(n, li.h_out, li.w_out, li.c_out).clone()

    def forward_timed(self, images: torch.Tensor, reps: int = 1) -> np.ndarray:
        """Per-layer milliseconds (HIP events on the launch stream), averaged over `reps`."""
        images = self._check_images(images)
        if images.dtype == torch.uint8:
            images = self._as_float32(images)
        n = images.shape[0]
        nl = self.lib.metro_plan_num_layers(self._plan)
        ms = (C.c_float * nl)()
        poses = torch.empty((n, self.spec.skeleton.n_out, 3), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for _ in range(reps):
            check(self.lib.metro_forward_timed(self._plan, C.c_void_p(images.data_ptr()), n,
                                               C.c_void_p(poses.data_ptr()),
                                               C.c_void_p(self._ws.data_ptr()), C.c_void_p(stream), ms),
                  'metro_forward_timed')
        return np.asarray(ms, dtype=np.float64) / reps

    def close(self) -> None:
        if self._plan:
            if self._ws is not None and self.device is not None:
                torch.cuda.synchronize(self.device)      # queued launches still read the plan's parameter blob / workspace
            self.lib.metro_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
