"""The launch contract of the C ABI and of the Python chains on a side stream (tests/stream_harness.py has the protocol).

Every launching entry takes a `void* stream`, every Python wrapper passes torch's current stream, and Engine.forward promises
"enqueued on torch's current stream; no synchronisation".  The rest of the suite calls the entries with the null stream (None,
or torch's current stream while that is the default one), so a launch, a memset or a graph launch that dropped its stream
argument, or a stray synchronisation, would pass it.  Here every entry runs once on a side stream the null stream does not
wait for (probed), behind a delay,
from inputs that are copied into place ON that stream after a decoy: work that lands on another stream reads the decoy and is
seen, a call that waits for the stream is seen too.

  TABLE       one case per prototype with a `void* stream` parameter (test_every_stream_entry_is_in_the_table, on the CPU:
              the two headers are parsed, a new entry cannot be added without a case).  Each case calls the builder an existing
              test or wrapper already has, once for the decoy A and once for B, and the harness records the C call it makes.
              The smallest shapes of those builders; index tensors are the same, valid ones in A and in B.
  EXEMPT      entries that synchronise by contract -- metro_forward_status, metro_forward_timed: their cases assert step 5 of
              the protocol only, the ordering and the bits.
  planted     the harness is shown to fail: a wrapper that passes stream 0, a wrapper that synchronises, a wrapper whose clear
              runs on stream 0 while its kernel runs on s.
  captured    metro_forward with metro_plan_set_graph_max_batch: first sight, capture, replay, and a replay on a second stream.
  chains      the Python calls under torch.cuda.stream(s), against the same call on the default stream.  Engine.forward and
              the heads wrappers (on device-resident arguments: a host array is uploaded from pageable memory, which waits
              for the stream) and preprocess.warp_crops must also return while the delay runs.  The frames chains,
              inference.estimate_pose, Follower.step and metrics.eval_metrics make one documented host synchronisation
              (the finite screen, a frame status, the metrics' sums): for them the ordering is proven for the launches in FRONT of that synchronisation
              only -- the delay is over once it returns -- and neither asynchrony nor a busy stream is asserted."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from metro_pose3d_amd._lib import check
from tests import helpers as H
from tests import stream_harness as SH

gpu = pytest.mark.gpu

EXEMPT = {
    'metro_forward_status': 'copies the status words to the host: synchronises the stream by contract (include/metro_hip.h)',
    'metro_forward_timed': 'reads its HIP events on the host after every layer: synchronises by contract',
}
H36M = ModelSpec(50, 32, 'h36m')
F16, F32 = _lib.METRO_F16, _lib.METRO_F32


def _rng(which, *tag):
    return np.random.default_rng([which == 'B', zlib.crc32(repr(tag).encode())])


class Ctx:
    """What the builders share in a session: the device, the libraries, the toy engines."""

    def __init__(self, dev, tmp):
        self.dev, self.tmp, self.lib, self._engines = dev, tmp, _lib.load(), {}

    def up(self, a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(self.dev)

    def model(self):
        if 'model' not in self._engines:
            from tests.test_gpu_placement import _toy_engine_model
            self._engines['model'] = _toy_engine_model(self.tmp)
        return self._engines['model']

    def engine(self, precision='f16', graphs=0):
        key = (precision, graphs)
        if key not in self._engines:
            from metro_pose3d_amd import Engine
            spec, params, _ = self.model()
            eng = Engine(spec, params, precision, max_batch=4, device=self.dev)
            check(self.lib.metro_plan_set_graph_max_batch(eng._plan, graphs), 'metro_plan_set_graph_max_batch')
            self._engines[key] = eng
        return self._engines[key]

    def images(self, which, n=2, u8=False):
        side = self.model()[0].proc_side
        a = _rng(which, 'images', n).integers(0, 256, (n, side, side, 3), dtype=np.uint8)
        return self.up(a) if u8 else self.up(a.astype(np.float32) / np.float32(255))


# ---- the table ---------------------------------------------------------------------------------------------------------------------

TABLE = []          # (entry, variant id, builder(ctx, which), options)


def case(entry, variant='', **options):
    def register(fn):
        TABLE.append((entry, variant, fn, options))
        return fn
    return register


# ---- convs
def _small(cases, prefix=''):
    """The smallest Case of a kernel family (tests/test_gpu_conv_contract.py) that helpers.run_conv_* can state."""
    fit = [c for c in cases if c.family.startswith(prefix) and not c.off and c.pix is None]
    return min(fit, key=lambda c: c.n * c.h * c.w * (c.c_in + c.c_out))


def _conv_f16_family(prefix):
    def build(ctx, which):
        from tests import test_gpu_conv_contract as CC
        c = _small(CC.CASES, prefix)
        d = c.desc()
        x, w, b, pro, res = CC._operands(c, d, _rng(which, 'conv_f16', c.name))
        H.run_conv_f16(ctx.lib, ctx.dev, d, x, w, b, pro, res)
    return build


for _family in ('conv3x3_c64', 'conv3x3_f16_slab<', 'conv_igemm_f16_dma<', 'conv_pw64<', 'conv_pws<', 'conv_gemm4w<'):
    case('metro_conv_f16', _family.rstrip('<'))(_conv_f16_family(_family))


@case('metro_conv_f64acc')
def _conv_f64acc(ctx, which):
    from tests import test_gpu_conv_contract as CC
    c = _small(CC.PRECISE)
    d = c.desc(in_dtype=F32, out=F32)
    x, w, b, _, res = CC._operands(c, d, _rng(which, 'f64acc', c.name))
    H.run_conv_f64acc(ctx.lib, ctx.dev, d, x, w, b, None, res)


@case('metro_conv_f32m')
def _conv_f32m(ctx, which):
    from tests import test_gpu_conv_contract as CC
    c = _small(CC.PRECISE)
    d = c.desc(in_dtype=F32, out=F32)
    x, w, b, _, res = CC._operands(c, d, _rng(which, 'f32m', c.name))
    t = [ctx.up(x, np.float32), ctx.up(w, np.float32), ctx.up(b, np.float32), None if res is None else ctx.up(res, np.float32)]
    out = torch.empty((d.n, d.h_out, d.w_out, d.c_out), dtype=torch.float32, device=ctx.dev)
    check(ctx.lib.metro_conv_f32m(C.byref(d), H.ptr(t[0]), H.ptr(t[1]), H.ptr(t[2]), None, None, H.ptr(t[3]), H.ptr(out), None), 'f32m')
    return t, out


def _nf_problem(builder, arg, vary, then=None):
    """A launch the non-finite tests already build (tests/test_gpu_nonfinite_kernels.py: Problem, Arena, _launch); the decoy has
    the tensors `vary` halved (exact in fp16 and fp32)."""
    def build(ctx, which):
        from tests import test_gpu_nonfinite_kernels as NF
        pr = getattr(NF, builder)(arg)
        if which == 'A':
            for name in vary:
                pr.tensors[name] = (pr.tensors[name].astype(np.float32) * np.float32(0.5)).astype(pr.tensors[name].dtype)
        if then is not None:
            then(pr)
        arena = NF.Arena(pr)
        base = torch.from_numpy(arena.host(False)).to(ctx.dev)
        NF._launch(ctx.lib, ctx.dev, pr, arena, base, [])
        return base
    return build


case('metro_conv_f16_pair')(_nf_problem('_build_pair', (2, 8, 64, 256, 64), ['x']))
case('metro_conv_f16_next')(_nf_problem('_build_next', (2, 8), ['x', 'res']))
case('metro_conv_f16_conv1_conv2')(_nf_problem('_build_conv1_conv2', (2, 16), ['x']))
case('metro_conv_f16_next_proj')(_nf_problem('_build_next_proj', (2, 8, 1), ['x', 'xu']))
case('metro_conv_f16_next_rebuild')(_nf_problem('_build_next_rebuild', (2, 16), ['x', 'xu', 'tp']))
case('metro_conv_f16_gemm4w')(_nf_problem('_build_gemm', ('gemm4w', 'k128'), ['x']))
case('metro_conv_f16_gemm8p', lib='experimental')(_nf_problem('_build_gemm', ('gemm8p', 'k128'), ['x']))
case('metro_conv_f16_gemm4d', lib='experimental')(_nf_problem('_build_gemm', ('gemm4d', 'k128'), ['x']))


def _geo_launch(pr):
    """G8_CASES' k128 through metro_conv_f16_gemm4d_geo (geometry 1), as tests/test_gpu_kernels.py::test_conv_gemm_experimental calls it."""
    n, _, _, c_in = pr.tensors['x'].shape
    c_out = pr.tensors['w'].shape[0]
    d = H.conv_desc(n, 16, c_in, 16, c_out, 1)

    def launch(lib, p, o, scratch):
        check(_lib.load_experimental().metro_conv_f16_gemm4d_geo(C.byref(d), p['x'], p['w'], p['b'], None, None, None, o[0], 0, None, 1, None),
              'metro_conv_f16_gemm4d_geo')
    pr.launch = launch


case('metro_conv_f16_gemm4d_geo', lib='experimental')(_nf_problem('_build_gemm', ('gemm4d', 'k128'), ['x'], then=_geo_launch))


# ---- stem, images, pool
def _stem_operands(ctx, which, n=2, side=64):
    rng = _rng(which, 'stem', n, side)
    img = rng.uniform(0, 1, (n, side, side, 3)).astype(np.float32)
    wp = np.zeros((64, 7, 8, 4), np.float16)
    wp[:, :, :7, :3] = (rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(np.float16)
    out = torch.empty((n, side // 4, side // 4, 64), dtype=torch.float16, device=ctx.dev)
    return ctx.up(img), ctx.up(wp), ctx.up((rng.standard_normal(64) * 0.5).astype(np.float32)), out


@case('metro_prep_input_f16')
def _prep_input(ctx, which):
    img = _stem_operands(ctx, which)[0]
    prepped = torch.empty((2, 70, 72, 4), dtype=torch.float16, device=ctx.dev)
    check(ctx.lib.metro_prep_input_f16(H.ptr(img), 2, 64, H.ptr(prepped), None), 'metro_prep_input_f16')
    return img, prepped


@case('metro_stem_pool_f16')
def _stem_f16(ctx, which):
    img, wp, b, out = _stem_operands(ctx, which)
    prepped = _prep_input(ctx, which)[1]            # (a real launch: only the entry under test is recorded)
    check(ctx.lib.metro_stem_pool_f16(H.ptr(prepped), H.ptr(wp), H.ptr(b), H.ptr(out), 2, 64, None), 'metro_stem_pool_f16')
    return prepped, wp, b, out


@case('metro_stem_pool_f32in')
def _stem_f32in(ctx, which):
    img, wp, b, out = _stem_operands(ctx, which)
    check(ctx.lib.metro_stem_pool_f32in(H.ptr(img), H.ptr(wp), H.ptr(b), H.ptr(out), 2, 64, None), 'metro_stem_pool_f32in')
    return img, wp, b, out


@case('metro_stem_pool_u8in')
def _stem_u8in(ctx, which):
    _, wp, b, out = _stem_operands(ctx, which)
    img = ctx.up(_rng(which, 'stem-u8').integers(0, 256, (2, 64, 64, 3), dtype=np.uint8))
    check(ctx.lib.metro_stem_pool_u8in(H.ptr(img), H.ptr(wp), H.ptr(b), H.ptr(out), 2, 64, None), 'metro_stem_pool_u8in')
    return img, wp, b, out


def _u8_to_f32(ctx, which):
    src = ctx.up(_rng(which, 'u8').integers(0, 256, 4096, dtype=np.uint8))
    out = torch.empty(4096, dtype=torch.float32, device=ctx.dev)
    check(ctx.lib.metro_images_u8_to_f32(H.ptr(src), 4096, H.ptr(out), None), 'metro_images_u8_to_f32')
    return src, out


case('metro_images_u8_to_f32')(_u8_to_f32)


@case('metro_maxpool3x3s2_zeropad')
def _maxpool(ctx, which):
    x = ctx.up(_rng(which, 'pool').standard_normal((2, 8, 8, 8)).astype(np.float16))
    out = torch.empty((2, 4, 4, 8), dtype=torch.float16, device=ctx.dev)
    check(ctx.lib.metro_maxpool3x3s2_zeropad(H.ptr(x), H.ptr(out), 2, 8, 8, 8, F16, None), 'metro_maxpool3x3s2_zeropad')
    return x, out


# ---- head and decode (side 8: one whole 64-pixel tile per image)
def _logits(which, n=2):
    from tests.test_gpu_heat_moments import random_logits
    return random_logits(H36M, n, 1.0, seed=int(which == 'B'))


@case('metro_softargmax')
def _softargmax(ctx, which):
    H.run_softargmax(ctx.lib, ctx.dev, H36M, _logits(which), 1)


@case('metro_softargmax01')
def _softargmax01(ctx, which):
    return MH.coords01_from_logits(ctx.up(_logits(which)), H36M, 1)


@case('metro_softargmax01_moments')
def _softargmax01_moments(ctx, which):
    return MH.moments_from_logits(ctx.up(_logits(which)), H36M, 1)


@case('metro_heat_marginals')
def _heat_marginals(ctx, which):
    return MH.marginals_from_logits(ctx.up(_logits(which)), H36M, 1)


@case('metro_heat_modes')
def _heat_modes(ctx, which):
    return MH.modes_from_logits(ctx.up(_logits(which)), H36M, 2, 1, 1)


@case('metro_heat_posterior')
def _heat_posterior(ctx, which):
    from tests.test_gpu_heat_posterior import make_prior
    return MH.posterior_from_logits(ctx.up(_logits(which)), make_prior(2, H36M.skeleton.n_out, ctx.dev, seed=3 + int(which == 'B')), H36M, 1)


case('metro_head_f16')(_nf_problem('_build_head', (H36M, 1), ['x']))


@case('metro_head_f16_moments')
def _head_moments(ctx, which):
    """tests/test_gpu_heat_moments.py::run_head's call ('plain64-one-record': c_in 320, side 8) on one image."""
    lib, spec, n, c_in, nj = ctx.lib, H36M, 1, 320, 17
    side, c = spec.heatmap_side, spec.n_head_channels
    rng = _rng(which, 'head-moments')
    t = [ctx.up(rng.standard_normal((n, side, side, c_in)).astype(np.float16)),
         ctx.up((rng.standard_normal((c, c_in)) * np.sqrt(2.0 / c_in)).astype(np.float16)), ctx.up((rng.standard_normal(c) * 0.1).astype(np.float32)),
         ctx.up(rng.uniform(0.5, 1.5, c_in).astype(np.float16)), ctx.up((rng.standard_normal(c_in) * 0.2).astype(np.float16))]
    cs = spec.to_c(_lib.METRO_PREC_F16)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=ctx.dev)
    scratch = torch.zeros(lib.metro_head_f16_scratch_bytes(n, side, nj), dtype=torch.uint8, device=ctx.dev)
    mscratch = torch.zeros(lib.metro_moments_scratch_bytes(C.byref(cs), n), dtype=torch.uint8, device=ctx.dev)
    outs = [f32(n, side, side, c), f32(n, spec.skeleton.n_out, 3), f32(n, nj, 3), f32(n, nj, 6), f32(n, nj)]
    check(lib.metro_head_f16_moments(*[H.ptr(a) for a in t], n, c_in, C.byref(cs), H.ptr(scratch), H.ptr(mscratch),
                                     *[H.ptr(o) for o in outs], None), 'metro_head_f16_moments')
    return t, scratch, mscratch, outs


# ---- warps: one 48 x 64 frame, two crops
WARP_BOXES = np.array([[4.0, 6, 30, 36], [20, 10, 40, 30]])
WARP_SIDE = 64


def _frame(ctx, which, nv12=False):
    shape = (72, 64) if nv12 else (48, 64, 3)
    return ctx.up(_rng(which, 'frame', nv12).integers(0, 256, shape, dtype=np.uint8))


@case('metro_warp_crop_u8')
def _warp_crop(ctx, which):
    from metro_pose3d_amd.preprocess import box_homography, warp_crops
    return warp_crops(_frame(ctx, which), np.stack([box_homography(b, WARP_SIDE) for b in WARP_BOXES]), WARP_SIDE)


def _warp_frames(crop_dtype, nv12):
    def build(ctx, which):
        fi = np.zeros(2, np.int64)
        params = FR.crop_params(None, WARP_BOXES, fi, WARP_SIDE)
        frame = _frame(ctx, which, nv12)
        return frame, FR.warp_frames([frame], params, fi, WARP_SIDE, device=ctx.dev, crop_dtype=crop_dtype,
                                     pixel_format='nv12' if nv12 else 'rgb')
    return build


case('metro_warp_crops_frames_u8')(_warp_frames('float32', False))
case('metro_warp_crops_frames_u8_to_u8')(_warp_frames('uint8', False))
case('metro_warp_crops_frames_planes', 'nv12')(_warp_frames('float32', True))
case('metro_warp_crops_frames_planes_to_u8', 'nv12')(_warp_frames('uint8', True))


# ---- geometry
def _rig_boxes(which):
    from tests import triangulation_ref as TR
    boxes = np.array([[300.0, 200, 220, 400], [900, 300, 260, 380]]) + (4.0 if which == 'A' else 0.0)
    return TR.ring_cameras([0, 90]), boxes, np.array([0, 1], np.int64)


@case('metro_expand_views')
def _expand_views(ctx, which):
    cams, boxes, fi = _rig_boxes(which)
    return FR._expand_views(FR.pack_view_bases(cams, boxes, fi, 256), FR.view_set(2), 256, ctx.dev)


@case('metro_look_at_boxes', sentinel=('d_status',))        # the status word is cleared by a memset in front of the kernel
def _look_at_boxes(ctx, which):
    cams, boxes, fi = _rig_boxes(which)
    return FR._look_at_boxes(cams, ctx.up(boxes), ctx.up(fi.astype(np.int32)), 2, 256, ctx.dev)


@case('metro_merge_views')
def _merge_views(ctx, which):
    cams, boxes, fi = _rig_boxes('B')
    sk, rng = H36M.skeleton, _rng(which, 'merge')
    _, places = FR._expand_views(FR.pack_view_bases(cams, boxes, fi, 256), FR.view_set(2), 256, ctx.dev)
    t = [ctx.up(rng.normal(0, 300, (4, sk.n_out, 3)).astype(np.float32)), ctx.up(rng.uniform(0, 256, (4, sk.n_out, 2)).astype(np.float32)),
         ctx.up(rng.uniform(3000, 5000, 4).astype(np.float32)), places, ctx.up(np.asarray(sk.out_mirror, np.int32))]
    return t, FR._merge_views(*t, 2, 2, True)


def _placement_fixture(which):
    """tests/golden/ref_placement_v1.npz (20 crops of 3 cameras); the decoy has coords01 drawn towards the crop centre."""
    from tests.test_placement import fixture_params
    d, q = fixture_params()
    c01 = d['coords01'].astype(np.float32)
    return d, q, (np.float32(0.5) + (c01 - np.float32(0.5)) * np.float32(0.9)) if which == 'A' else c01


@case('metro_place_poses')
def _place_poses(ctx, which):
    from tests import test_gpu_placement as GPL
    d, q, c01 = _placement_fixture(which)
    GPL._place(ctx.dev, GPL.SPEC, c01, q, 'bone-lengths', 'world', bones=d['bone_targets'])


@case('metro_place_covariances')
def _place_covariances(ctx, which):
    from tests import triangulation_ref as TR
    d, q, _ = _placement_fixture(which)
    n, nj, rng = len(d['coords01']), H36M.skeleton.n_head, _rng(which, 'place-cov')
    cov01 = np.asarray(TR.cov01_for(rng.uniform(0.5, 30.0, (n, nj)), H36M, (n, nj)), np.float32)
    return MH.place_covariances(ctx.up(cov01), ctx.up(rng.uniform(0.1, 1.0, (n, nj)).astype(np.float32)), H36M, 'world',
                                ctx.up(FR.pack_placements(q)).reshape(-1), 1)


@case('metro_backproject_bone_lengths')
def _backproject_bones(ctx, which):
    d, q, c01 = _placement_fixture(which)
    return MH.backproject_bone_lengths(ctx.up(c01), q.inv_intrinsics, d['bone_targets'], H36M, permute=True)


@case('metro_backproject_root_depth')
def _backproject_root(ctx, which):
    d, q, c01 = _placement_fixture(which)
    return MH.backproject_root_depth(ctx.up(c01), q.inv_intrinsics, d['root_depth'], H36M)


@case('metro_heatmap_to_25d')
def _to_25d(ctx, which):
    return MH.heatmap_to_25d(ctx.up(_placement_fixture(which)[2]), H36M)


@case('metro_to_orig_cam')
def _to_orig_cam(ctx, which):
    d, q, _ = _placement_fixture(which)
    rel = d['metro_crop'][:, list(H36M.skeleton.permutation)].astype(np.float32) * np.float32(0.5 if which == 'A' else 1.0)
    return MH.to_orig_cam(ctx.up(rel), q.rot_to_orig_cam, H36M.skeleton.out_mirror)


@case('metro_eval_metrics')
def _eval_metrics(ctx, which):
    from metro_pose3d_amd.metrics import eval_metrics
    rng = _rng(which, 'metrics')
    true = rng.normal(0, 300, (2, 17, 3)).astype(np.float32)
    with np.errstate(all='ignore'):                 # (the recorded call launches nothing: the wrapper's means are of unwritten sums)
        return eval_metrics(ctx.up(true + rng.normal(0, 30, true.shape).astype(np.float32)), ctx.up(true))


# ---- multi-view
def _device_case(ctx, c):
    return ctx.up(c['coords01']), ctx.up(c['cov01']), ctx.up(FR.pack_placements(c['places'])).reshape(-1)


def _jitter(which, coords01, spec):
    """Two pixels of noise on the heat-map positions, drawn per input set."""
    from tests import triangulation_ref as TR
    c = np.array(coords01, np.float32)
    c[..., :2] += _rng(which, 'jitter').normal(0, 2.0 / TR.pixel_scale(spec)[0], c[..., :2].shape).astype(np.float32)
    return c


def _triangulate(return_covariance):
    def build(ctx, which):
        from tests import triangulation_ref as TR
        s = TR.ring_scene([0, 120, 240], 3, H36M, seed=2)            # 3 persons, 3 cameras
        n, nj = len(s['boxes']), H36M.skeleton.n_head
        rows, starts = FR.person_groups(s['pi'], s['fi'])
        c = TR.case(_jitter(which, s['coords01'], H36M), TR.cov01_for(np.ones((n, nj)), H36M, (n, nj)), s['places'], rows, starts, 'covariance')
        return MH.triangulate_joints(*_device_case(ctx, c), c['rows'], c['starts'], H36M, 'covariance', return_covariance=return_covariance)
    return build


case('metro_triangulate_joints')(_triangulate(False))
case('metro_triangulate_joints_cov')(_triangulate(True))


def _affinity(steps):
    def build(ctx, which):
        from tests import match_views_ref as MR
        c = MR.CASES['rig-2x1'](H36M, 'covariance')
        c['coords01'] = _jitter(which, c['coords01'], H36M)
        tail = (H36M, c['n_views'], c['weights'], c['min_angle_deg'], c['clip_mm'], c['min_joints'])
        if steps:
            return MH.view_affinity_steps(*_device_case(ctx, c), c['fi'], np.zeros(len(c['fi']), np.int32), *tail)
        return MH.view_affinity(*_device_case(ctx, c), c['fi'], *tail)
    return build


case('metro_view_affinity', 'rig-2x1')(_affinity(False))
case('metro_view_affinity_steps', 'rig-2x1')(_affinity(True))


@case('metro_cluster_views')
def _cluster_views(ctx, which):
    from tests import match_views_ref as MR
    return MH.cluster_views(ctx.up(np.asarray(MR.random_cost(4, seed=11 + (which == 'B')), np.float32)), 200.0, 1)


@case('metro_person_steps', 'n64-s2')
def _person_steps(ctx, which):
    from tests import world_follow_ref as WR
    c = WR.person_steps_cases()['n64-s2']
    return MH.person_steps(ctx.up(c['rows']), ctx.up(c['starts']), ctx.up(np.asarray([c['n_persons']], np.int32)), c['box_step'],
                           c['step_times'] + (which == 'A'), c['n_views'])


@case('metro_person_steps_labels', 'n2-pair')
def _person_steps_labels(ctx, which):
    from tests import single_view_ref as SV
    c = SV.labels_cases()['n2-pair']
    return MH.person_steps_labels(ctx.up(np.asarray(c['person_index'], np.int32)), ctx.up(np.asarray([c['n_persons']], np.int32)),
                                  c['box_step'], np.asarray(c['step_times'], np.float64) + (which == 'A'))


@case('metro_person_rays', 'P9-J7-V2')
def _person_rays(ctx, which):
    from tests import single_view_ref as SV
    c, _ = SV.rays_case_and_expected('P9-J7-V2-covariance')
    c01 = np.asarray(c['coords01'], np.float32)
    if which == 'A':
        c01 = np.float32(0.5) + (c01 - np.float32(0.5)) * np.float32(0.9)
    return MH.person_rays(ctx.up(c01), ctx.up(c['cov01']), ctx.up(FR.pack_placements(c['places'])).reshape(-1), ctx.up(c['single_box']),
                          c['spec'], c['n_views'], c['weights'])


# ---- tracking: the in-place tables (state, ids, next_id, poses and covariance of the ray entry, the bone table) are in-out
def _moved(which, poses):
    return np.asarray(poses, np.float32) * np.float32(1.001 if which == 'A' else 1.0)


@case('metro_smooth_tracks', 'ragged')
def _smooth_tracks(ctx, which):
    from tests import test_gpu_track_smoothing as GTS, track_smoothing_ref as TS
    c = dict(TS.case_and_expected('ragged', 'smooth', 'covariance')[0])       # (the cases are cached: a copy takes the decoy)
    c['poses'] = _moved(which, c['poses'])
    GTS._launch(c, ctx.dev)


@case('metro_associate_tracks', 'cap1-box2')
def _associate(ctx, which):
    from tests import follow_tracks_ref as FT, test_gpu_follow_tracks as GFT
    c = dict(FT.case_and_expected('cap1-box2')[0])
    c['poses'] = _moved(which, c['poses'])
    GFT._launch(c, ctx.dev)


@case('metro_associate_tracks_optimal', 'followed-cap1-box2')
def _associate_optimal(ctx, which):
    from tests import assign_tracks_ref as AR, test_gpu_assign_tracks as GAT
    c = dict(AR.case_and_expected('followed-cap1-box2')[0])
    c['poses'] = _moved(which, c['poses'])
    GAT._launch(c, ctx.dev)


@case('metro_associate_tracks_rays', 'T1-m1-ray-only-step')
def _associate_rays(ctx, which):
    from tests import single_view_ref as SV
    c = SV.case('T1-m1-ray-only-step')
    state, ids, next_id = ctx.up(c['state']), ctx.up(c['ids']), ctx.up(np.asarray(c['next_id'], np.int32).reshape(1))
    return state, ids, next_id, MH.associate_tracks_rays(
        ctx.up(_moved(which, c['poses'])), ctx.up(c['cov']), c['times'], c['step_rows'], c['step_starts'], state, ids, next_id,
        ctx.up(c['single_box']), ctx.up(c['rays']), c['max_cost'], c['clip'], c['min_joints'], c['max_age'], c['q'], c['r_floor'],
        c['cov_scale'], c['v0'], None, 'greedy', c['depth_sigma'])


@case('metro_track_bone_lengths', 'T2-E16-J17')
def _bone_lengths(ctx, which):
    from tests import bone_lengths_ref as BL
    c = BL.shape_case('T2-E16-J17')
    call = c['calls'][0]
    table = FR.new_bone_table(c['T'], len(c['edges']), ctx.dev)
    return table, MH.track_bone_lengths(ctx.up(_moved(which, call['poses'])), None if call['cov'] is None else ctx.up(call['cov']),
                                        call['rows'], call['starts'], ctx.up(call['ids']), table.stats, table.ids, c['edges'], c['mirror'],
                                        c['fallback'], **c['params'])


@case('metro_predict_boxes', 'standing')
def _predict_boxes(ctx, which):
    from tests import predict_boxes_ref as PB
    c = PB.CASES['standing']()
    c = c[0] if isinstance(c, tuple) else c
    p = PB.params_of(c)
    state = np.array(c['state'], np.float64)
    state[..., :3] += 3.0 * (which == 'A')                      # free slots stay NaN
    # host arrays the entry reads through pointers: of the dtype and layout the wrapper passes on as they are, and kept alive
    sizes, times = np.ascontiguousarray(c['sizes'], np.int32), np.ascontiguousarray(c['times'], np.float64)
    rows = MH.predict_boxes(ctx.up(state), ctx.up(np.asarray(c['ids'], np.int32)), FR.pack_frame_cameras(c['cameras']), sizes, times,
                            c['coords'], None, None, p['expand'], p['n_sigma'], p['max_sigma'], p['min_joints'], p['max_age'], p['near'],
                            p['min_side'], p['iou_max'], p['q'], p['clip'])
    return sizes, times, rows


# ---- forwards: the toy model of tests/test_gpu_placement.py, two crops, f16
@case('metro_forward')
def _forward(ctx, which):
    return ctx.engine().forward(ctx.images(which))


@case('metro_forward_coords01')
def _forward_coords01(ctx, which):
    eng = ctx.engine()
    c01 = torch.empty((2, eng.spec.skeleton.n_head, 3), dtype=torch.float32, device=ctx.dev)
    return c01, eng.forward(ctx.images(which), coords01=c01)


@case('metro_forward_u8')
def _forward_u8(ctx, which):
    return ctx.engine().forward(ctx.images(which, u8=True))


@case('metro_forward_moments')
def _forward_moments(ctx, which):
    eng = ctx.engine()
    nj = eng.spec.skeleton.n_head
    outs = [torch.empty(s, dtype=torch.float32, device=ctx.dev) for s in ((2, nj, 3), (2, nj, 6), (2, nj))]
    return outs, eng.forward(ctx.images(which), coords01=outs[0], cov01=outs[1], peak=outs[2])


def _middle_layer(eng):
    infos = eng.layer_infos()
    return next(i for i in range(len(infos) // 2, len(infos)) if infos[i].kind == _lib.LAYER_CONV)


def _upto_tensor(ctx):
    """The middle layer's tensor inside the workspace: compared although the workspace as a whole is scratch."""
    eng = ctx.engine()
    li = eng.layer_infos()[_middle_layer(eng)]
    return [('d_workspace', int(li.out_offset), int(li.out_bytes_per_image) * 2)]


@case('metro_forward_upto', 'middle-layer', extra=_upto_tensor)
def _forward_upto(ctx, which):
    eng = ctx.engine()
    return eng.forward_upto(ctx.images(which), _middle_layer(eng))


@case('metro_forward_timed', synchronises=True)
def _forward_timed(ctx, which):
    return ctx.engine().forward_timed(ctx.images(which))


class _StatusCall(SH.RecordedCall):
    """metro_forward_status: its input is the status words a forward left in the workspace (A: none set, B: crop 1 flagged), its
    outputs are on the host: the return value and *n_nonfinite_out."""

    def __init__(self, ctx, *args):
        super().__init__(*args)
        off = int(ctx.lib.metro_plan_status_offset(ctx.engine()._plan))
        ws, at = self.rec.pointers[1]
        for which, words in (('A', [0, 0]), ('B', [0, 1])):
            self.stage[which][ws][at + off:at + off + 8] = torch.tensor(words, dtype=torch.int32).view(torch.uint8).to(ctx.dev)
        self.dev = ctx.dev

    def check_status(self):
        assert self.status in (0, -5), f'{self.entry}: status {self.status}'

    def snapshot(self):
        return [torch.tensor([self.status & 0xFF, self.rec.args[4]._obj.value & 0xFF], dtype=torch.uint8).to(self.dev)]

    def pure(self):
        return [False]


@case('metro_forward_status', synchronises=True, subject=_StatusCall)
def _forward_status(ctx, which):
    eng = ctx.engine()
    eng.forward(ctx.images(which))
    eng.check_finite(2)


CASE_IDS = [f'{entry}[{variant}]' if variant else entry for entry, variant, _, _ in TABLE]


# ---- the closure, on the CPU -------------------------------------------------------------------------------------------------------

def test_every_stream_entry_is_in_the_table():
    """Every prototype of the two headers with a `void* stream` parameter is named by the cases of exactly one builder family of
    the table (metro_conv_f16 has one variant per kernel family, every other entry one case); the entries that synchronise by
    contract are those in EXEMPT, each with its reason, and their cases assert the ordering and the bits only."""
    entries = SH.stream_entries()
    assert len(entries) >= 59 and sum(name in _lib.EXPERIMENTAL_SIGNATURES for name in entries) >= 3, sorted(entries)
    named = [entry for entry, _, _, _ in TABLE]
    assert set(named) == set(entries), (sorted(set(entries) - set(named)), sorted(set(named) - set(entries)))
    assert len(CASE_IDS) == len(set(CASE_IDS))
    for entry in entries:
        variants = [v for e, v, _, _ in TABLE if e == entry]
        assert len(variants) == 1 or entry == 'metro_conv_f16', (entry, variants)
    synchronising = {entry for entry, _, _, opt in TABLE if opt.get('synchronises')}
    assert synchronising == set(EXEMPT) == {'metro_forward_status', 'metro_forward_timed'}
    assert all(isinstance(r, str) and r and '\n' not in r for r in EXEMPT.values())
    for entry, params in entries.items():              # what the harness reads from the prototypes
        sig = (_lib.EXPERIMENTAL_SIGNATURES if entry in _lib.EXPERIMENTAL_SIGNATURES else _lib.SIGNATURES)[entry][1]
        assert len(sig) == len(params) and all(p.name for p in params), entry
        assert all(p.pointer for p, ty in zip(params, sig) if ty is C.c_void_p), entry


def test_prototype_roles():
    roles = {p.name: p.role for p in SH.stream_entries()['metro_associate_tracks_rays']}
    assert (roles['d_poses'], roles['d_cov'], roles['d_state'], roles['d_ids'], roles['d_next_id']) == ('inout',) * 5
    assert (roles['d_times'], roles['d_workspace'], roles['d_cost_out'], roles['n'], roles['d_rays']) == ('in', 'scratch', 'out', 'value', 'in')
    bones = {p.name: p.role for p in SH.stream_entries()['metro_track_bone_lengths']}
    assert (bones['d_stats'], bones['d_bone_ids'], bones['d_lengths_out'], bones['d_ids']) == ('inout', 'inout', 'out', 'in')
    conv = {p.name: p.role for p in SH.stream_entries()['metro_conv_f16_next_rebuild']}
    assert (conv['d_out'], conv['d_out_sub'], conv['d_out2'], conv['d_w2']) == ('out', 'out', 'out', 'in')


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ctx(cuda, tmp_path_factory):
    c = Ctx(cuda, tmp_path_factory.mktemp('streams'))
    c.engine()              # bound before anything is recorded: the parameter blob is no input of a call
    return c


def _subject(ctx, entry, build, options):
    lib = _lib.load_experimental() if options.get('lib') == 'experimental' else ctx.lib
    params = SH.stream_entries()[entry]
    rec = {which: SH.record(lib, entry, params, lambda which=which: build(ctx, which)) for which in ('A', 'B')}
    extra = options['extra'](ctx) if 'extra' in options else ()
    if 'subject' in options:
        return options['subject'](ctx, lib, entry, params, rec['A'], rec['B'], extra)
    return SH.RecordedCall(lib, entry, params, rec['A'], rec['B'], extra, options.get('sentinel', ()))


@gpu
@pytest.mark.parametrize('entry,variant,build,options', TABLE, ids=CASE_IDS)
def test_entry_keeps_to_its_stream(ctx, entry, variant, build, options):
    """The protocol of tests/stream_harness.py on one C entry: on a non-blocking side stream, behind a delay of
    max(50 ms, 20 T), from inputs copied into place on that stream, the call returns while the delay runs, leaves the stream
    busy, and its outputs have the bits of the default-stream run on the same inputs."""
    subject = _subject(ctx, entry, build, options)
    v = SH.verdict(subject, ctx.dev, what=f'{entry} {variant}'.strip(), asynchronous=not options.get('synchronises'))
    v.require_ok()


def _cheap_subject(ctx):
    entry = 'metro_images_u8_to_f32'
    return _subject(ctx, entry, _u8_to_f32, {})


@gpu
def test_planted_wrong_stream_is_reported_as_running_ahead(ctx):
    """A wrapper that drops its stream argument (passes 0) while B is produced on s: the kernel runs on the null stream at once,
    on the decoy -- want_A's bits, 'work ran ahead of its stream'."""
    v = SH.verdict(_cheap_subject(ctx), ctx.dev, what='planted: stream 0', wrap=lambda subject, s: subject.run(0))
    print(f'side stream variant: {SH.stream_variant()}')
    assert v.kind == 'ran-ahead' and 'want_A' in v.message and 'mixture' not in v.message, (v.kind, v.message)
    assert SH._same(v.detail['early'], v.detail['want']['A']), 'seen while the delay still ran'


@gpu
def test_planted_synchronisation_is_reported(ctx):
    """A wrapper that synchronises the stream before it returns: 'the call synchronised', whatever the bits."""
    def wrap(subject, s):
        subject.run(s.cuda_stream)
        s.synchronize()
    v = SH.verdict(_cheap_subject(ctx), ctx.dev, what='planted: hidden synchronisation', wrap=wrap)
    assert v.kind == 'synchronised' and 'the call synchronised' in v.message, (v.kind, v.message)


class _ClearThenAdd:
    """out = 0, then out += x: a clear in front of a kernel that only adds, as metro_look_at_boxes' memset of its status word in
    front of a kernel that only counts.  rogue: the clear goes to the default stream, the kernel to the call's stream."""

    def __init__(self, dev, rogue):
        self.dev, self.rogue = dev, rogue
        self.x = {w: torch.arange(64, dtype=torch.int32, device=dev) + (7 if w == 'B' else 1000) for w in 'AB'}
        self.work, self.out = self.x['A'].clone(), torch.zeros(64, dtype=torch.int32, device=dev)

    def fill(self, which):
        self.work.copy_(self.x[which], non_blocking=True)

    def poison(self):
        self.out.view(torch.uint8).fill_(SH.SENTINEL_BYTE)

    def run(self, stream_ptr):
        with torch.cuda.stream(torch.cuda.default_stream(self.dev) if self.rogue else torch.cuda.current_stream(self.dev)):
            self.out.zero_()
        self.out.add_(self.work)

    def check_status(self):
        pass

    def snapshot(self):
        return [self.out.view(torch.uint8).clone()]

    def pure(self):
        return [True]


@gpu
def test_planted_clear_on_the_wrong_stream_is_reported(ctx):
    """A clear whose effect is the same for A and B: on the default stream it runs ahead of the delay.  The outputs are seen to
    change while the delay runs, and since the sentinel is laid again on s the kernel then adds to the sentinel, not to zero: the
    final bits are wrong too.  The same subject with its clear on s passes."""
    SH.verdict(_ClearThenAdd(ctx.dev, rogue=False), ctx.dev, what='clear and kernel on s').require_ok()
    v = SH.verdict(_ClearThenAdd(ctx.dev, rogue=True), ctx.dev, what='planted: clear on stream 0, kernel on s')
    assert v.kind == 'ran-ahead' and 'while the delay' in v.message, (v.kind, v.message)
    assert not SH._same(v.detail['got'], v.detail['want']['B']), 'and the final bits are wrong as well'


@gpu
def test_captured_forward_keeps_to_the_stream_of_each_call(ctx):
    """metro_plan_set_graph_max_batch(plan, 4): three calls of one key on s -- the eager first sight, the capture, the replay --
    and a fourth, a replay, on a SECOND side stream (the cache key holds no stream), each through the whole protocol, each with
    the bits of the eager default-stream run (computed with graphs off).  The graph is a linear chain: no parallel branches."""
    eng = ctx.engine('f16', graphs=4)
    params = SH.stream_entries()['metro_forward']
    out = torch.empty((2, eng.spec.skeleton.n_out, 3), dtype=torch.float32, device=ctx.dev)      # one key: the same buffers
    rec = {which: SH.record(ctx.lib, 'metro_forward', params, lambda which=which: eng.forward(ctx.images(which), out=out)) for which in 'AB'}
    subject = SH.RecordedCall(ctx.lib, 'metro_forward', params, rec['A'], rec['B'])
    check(ctx.lib.metro_plan_set_graph_max_batch(eng._plan, 0), 'metro_plan_set_graph_max_batch')
    reference = SH.reference_run(subject, ctx.dev, 'metro_forward, graphs off')
    check(ctx.lib.metro_plan_set_graph_max_batch(eng._plan, 4), 'metro_plan_set_graph_max_batch')
    second = SH.side_stream(ctx.dev, second=True)
    for call, stream, launches in (('first sight', None, True), ('capture', None, True), ('replay', None, False),
                                   ('replay on a second stream', second, False)):
        # metro_kernel_notes(1): every launcher the call goes through appends its kernel id -- the eager first sight and the
        # capture walk the layers, a replay is one hipGraphLaunch and goes through none
        check(ctx.lib.metro_kernel_notes(1), 'metro_kernel_notes')
        try:
            v = SH.verdict(subject, ctx.dev, stream=stream, what=f'captured metro_forward, {call}', reference=reference)
            noted = ctx.lib.metro_last_kernel_id().decode()
        finally:
            ctx.lib.metro_kernel_notes(0)
        v.require_ok()
        assert bool(noted) == launches, f'{call}: ' + ('no launcher ran' if launches else f'not a replay, launchers ran: {noted[:80]}')


# ---- the Python chains -------------------------------------------------------------------------------------------------------------

def _chain(ctx, fn, a, b, what, asynchronous):
    SH.verdict(SH.Chain(fn, a, b), ctx.dev, what=what, asynchronous=asynchronous, busy=False).require_ok()


@gpu
@pytest.mark.parametrize('precision', ['f16', 'f64'])
@pytest.mark.parametrize('call', ['fp32', 'uint8', 'coords01', 'moments'])
def test_engine_forward_on_a_side_stream(ctx, call, precision):
    """Engine.forward under torch.cuda.stream(s): "enqueued on torch's current stream; no synchronisation" -- it returns while the
    delay in front of it runs, and poses (coords01, cov01, peak) have the bits of the call on the default stream."""
    eng = ctx.engine(precision)
    nj = eng.spec.skeleton.n_head
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=ctx.dev)

    def fn(images):
        if call == 'coords01':
            c01 = f32(2, nj, 3)
            return eng.forward(images, coords01=c01), c01
        if call == 'moments':
            outs = [f32(2, nj, 3), f32(2, nj, 6), f32(2, nj)]
            return eng.forward(images, coords01=outs[0], cov01=outs[1], peak=outs[2]), outs
        return eng.forward(images)
    u8 = call == 'uint8'
    _chain(ctx, fn, [ctx.images('A', u8=u8)], [ctx.images('B', u8=u8)], f'Engine.forward {call} {precision}', True)


def _heads_calls(ctx):
    """name -> (A inputs, B inputs, fn): heads wrappers on device-resident inputs."""
    from tests import match_views_ref as MR, track_smoothing_ref as TS, triangulation_ref as TR
    up, calls = ctx.up, {}
    calls['coords01_from_logits'] = ([up(_logits('A'))], [up(_logits('B'))], lambda lg: MH.coords01_from_logits(lg, H36M, 1))
    calls['moments_from_logits'] = ([up(_logits('A'))], [up(_logits('B'))], lambda lg: MH.moments_from_logits(lg, H36M, 1))
    calls['heatmap_to_25d'] = ([up(_placement_fixture('A')[2])], [up(_placement_fixture('B')[2])], lambda c: MH.heatmap_to_25d(c, H36M))
    d, q, _ = _placement_fixture('B')
    n, nj = len(d['coords01']), H36M.skeleton.n_head
    places = up(FR.pack_placements(q)).reshape(-1)
    cov = {w: [up(np.asarray(TR.cov01_for(_rng(w, 'cov').uniform(0.5, 30.0, (n, nj)), H36M, (n, nj)), np.float32)),
               up(_rng(w, 'peak').uniform(0.1, 1.0, (n, nj)).astype(np.float32))] for w in 'AB'}
    calls['place_covariances'] = (cov['A'], cov['B'], lambda c, p: MH.place_covariances(c, p, H36M, 'world', places, 1))
    rel = {w: d['metro_crop'][:, list(H36M.skeleton.permutation)].astype(np.float32) * np.float32(0.5 if w == 'A' else 1.0) for w in 'AB'}
    rot = up(np.asarray(q.rot_to_orig_cam, np.float32))
    calls['to_orig_cam'] = ([up(rel['A'])], [up(rel['B'])], lambda x: MH.to_orig_cam(x, rot, H36M.skeleton.out_mirror))
    inv_k, root = up(np.asarray(q.inv_intrinsics, np.float32)), up(np.asarray(d['root_depth'], np.float32))
    calls['backproject_root_depth'] = ([up(_placement_fixture('A')[2])], [up(_placement_fixture('B')[2])],
                                       lambda c: MH.backproject_root_depth(c, inv_k, root, H36M))
    calls['cluster_views'] = ([up(np.asarray(MR.random_cost(4, seed=11), np.float32))], [up(np.asarray(MR.random_cost(4, seed=12), np.float32))],
                              lambda c: MH.cluster_views(c, 200.0, 1))
    s = TR.ring_scene([0, 120, 240], 3, H36M, seed=2)
    m = len(s['boxes'])
    rows, starts = (up(np.asarray(a, np.int32)) for a in FR.person_groups(s['pi'], s['fi']))
    tri_places = up(FR.pack_placements(s['places'])).reshape(-1)
    tri_cov = up(np.asarray(TR.cov01_for(np.ones((m, nj)), H36M, (m, nj)), np.float32))
    calls['triangulate_joints'] = ([up(_jitter('A', s['coords01'], H36M))], [up(_jitter('B', s['coords01'], H36M))],
                                   lambda c: MH.triangulate_joints(c, tri_cov, tri_places, rows, starts, H36M, 'covariance', return_covariance=True))
    fi = up(np.asarray(s['fi'], np.int32))
    step = up(np.zeros(len(s['fi']), np.int32))
    calls['view_affinity_steps'] = ([up(_jitter('A', s['coords01'], H36M))], [up(_jitter('B', s['coords01'], H36M))],
                                    lambda c: MH.view_affinity_steps(c, tri_cov, tri_places, fi, step, H36M))
    calls['view_affinity'] = ([up(_jitter('A', s['coords01'], H36M))], [up(_jitter('B', s['coords01'], H36M))],
                              lambda c: MH.view_affinity(c, tri_cov, tri_places, fi, H36M))
    c, _ = TS.case_and_expected('ragged', 'smooth', 'covariance')
    t = [up(np.asarray(c['times'], np.float64)), up(np.asarray(c['rows'], np.int32)), up(np.asarray(c['starts'], np.int32))]
    track_cov = up(c['cov'])
    calls['smooth_tracks'] = ([up(_moved('A', c['poses']))], [up(_moved('B', c['poses']))],
                              lambda p: MH.smooth_tracks(p, track_cov, *t, c['mode'], c['measurement'], c['q'], c['r_floor'], c['cov_scale'], c['v0'], None))
    bone_targets = up(np.asarray(d['bone_targets'], np.float64))
    calls['backproject_bone_lengths'] = ([up(_placement_fixture('A')[2])], [up(_placement_fixture('B')[2])],
                                         lambda c: MH.backproject_bone_lengths(c, inv_k, bone_targets, H36M, permute=True))
    from tests import bone_lengths_ref as BL, follow_tracks_ref as FT, predict_boxes_ref as PB, single_view_ref as SV, world_follow_ref as WR
    ps = WR.person_steps_cases()['n64-s2']
    ps_dev = [up(ps['rows']), up(ps['starts']), up(np.asarray([ps['n_persons']], np.int32)), up(np.asarray(ps['box_step'], np.int32))]
    calls['person_steps'] = ([up(ps['step_times'] + 1.0)], [up(ps['step_times'])], lambda st: MH.person_steps(*ps_dev, st, ps['n_views']))
    lc = SV.labels_cases()['n2-pair']
    labels = [up(np.asarray(lc['person_index'], np.int32)), up(np.asarray([lc['n_persons']], np.int32)), up(np.asarray(lc['box_step'], np.int32))]
    times = np.asarray(lc['step_times'], np.float64)
    calls['person_steps_labels'] = ([up(times + 1.0)], [up(times)], lambda st: MH.person_steps_labels(*labels, st))
    ac = SV.case('T1-m1-ray-only-step')
    ray_table = [up(ac['state']), up(np.asarray(ac['ids'], np.int32)), up(np.asarray(ac['next_id'], np.int32).reshape(1))]
    ray_steps = [up(np.asarray(ac['times'], np.float64)), up(np.asarray(ac['step_rows'], np.int32)), up(np.asarray(ac['step_starts'], np.int32))]
    ray_in = [up(ac['cov']), up(np.asarray(ac['single_box'], np.int32)), up(ac['rays'])]

    def associate_rays(p):
        table = [x.clone() for x in ray_table]
        return MH.associate_tracks_rays(p, ray_in[0], *ray_steps, *table, ray_in[1], ray_in[2], ac['max_cost'], ac['clip'], ac['min_joints'],
                                        ac['max_age'], ac['q'], ac['r_floor'], ac['cov_scale'], ac['v0'], None, 'greedy', ac['depth_sigma']), table
    calls['associate_tracks_rays'] = ([up(_moved('A', ac['poses']))], [up(_moved('B', ac['poses']))], associate_rays)
    rc, _ = SV.rays_case_and_expected('P9-J7-V2-covariance')
    ray_dev = [up(rc['cov01']), up(FR.pack_placements(rc['places'])).reshape(-1), up(np.asarray(rc['single_box'], np.int32))]
    c01 = np.asarray(rc['coords01'], np.float32)
    calls['person_rays'] = ([up(np.float32(0.5) + (c01 - np.float32(0.5)) * np.float32(0.9))], [up(c01)],
                            lambda x: MH.person_rays(x, *ray_dev, rc['spec'], rc['n_views'], rc['weights']))
    fc = FT.case_and_expected('cap1-box2')[0]
    table0 = [up(np.asarray(fc['state'], np.float64)), up(np.asarray(fc['ids'], np.int32)), up(np.asarray(fc['next_id'], np.int32).reshape(1))]
    steps = [up(np.asarray(fc['times'], np.float64)), up(np.asarray(fc['step_rows'], np.int32)), up(np.asarray(fc['step_starts'], np.int32))]
    box_cov = up(np.asarray(fc['cov'], np.float32))

    def associate(assignment):
        def fn(p):
            table = [x.clone() for x in table0]            # the table is updated in place: a fresh copy per call, returned with the rest
            return MH.associate_tracks(p, box_cov, *steps, *table, fc['max_cost'], fc['clip'], fc['min_joints'], fc['max_age'], fc['measurement'],
                                       fc['q'], fc['r_floor'], fc['cov_scale'], fc['v0'], None, assignment), table
        return fn
    for rule in MH.ASSIGNMENTS:
        calls[f'associate_tracks-{rule}'] = ([up(_moved('A', fc['poses']))], [up(_moved('B', fc['poses']))], associate(rule))
    bc = BL.shape_case('T2-E16-J17')
    call = bc['calls'][0]
    bone_dev = [None if call['cov'] is None else up(call['cov']), up(np.asarray(call['rows'], np.int32)), up(np.asarray(call['starts'], np.int32)),
                up(np.asarray(call['ids'], np.int32))]

    def bones(p):
        table = FR.new_bone_table(bc['T'], len(bc['edges']), ctx.dev)
        return MH.track_bone_lengths(p, *bone_dev, table.stats, table.ids, bc['edges'], bc['mirror'], bc['fallback'], **bc['params']), table
    calls['track_bone_lengths'] = ([up(_moved('A', call['poses']))], [up(_moved('B', call['poses']))], bones)
    pc = PB.CASES['standing']()
    pc = pc[0] if isinstance(pc, tuple) else pc
    pp = PB.params_of(pc)
    cams = up(np.ascontiguousarray(FR.pack_frame_cameras(pc['cameras'])).view(np.uint8).reshape(-1, MH.FRAME_CAMERA_BYTES))
    slots, sizes = up(np.asarray(pc['ids'], np.int32)), np.ascontiguousarray(pc['sizes'], np.int32)
    state = np.array(pc['state'], np.float64)
    moved = state.copy()
    moved[..., :3] += 3.0

    def predict(st):
        r = MH.predict_boxes(st, slots, cams, sizes, pc['times'], pc['coords'], None, None, pp['expand'], pp['n_sigma'], pp['max_sigma'],
                             pp['min_joints'], pp['max_age'], pp['near'], pp['min_side'], pp['iou_max'], pp['q'], pp['clip'])
        # the rows come back unsliced: only the first counts[0] are written, the rest is whatever the allocation held
        written = torch.arange(len(r.boxes), device=ctx.dev) < r.counts[0]
        cut = lambda t: torch.where(written.view(-1, *[1] * (t.dim() - 1)), t, torch.zeros_like(t))
        return [cut(t) for t in r[:6]], r.dense_boxes, r.dense_joints, r.counts
    calls['predict_boxes'] = ([up(moved)], [up(state)], predict)
    return calls


HEADS_CALLS = ['coords01_from_logits', 'moments_from_logits', 'heatmap_to_25d', 'place_covariances', 'to_orig_cam', 'backproject_root_depth',
               'backproject_bone_lengths', 'cluster_views', 'triangulate_joints', 'view_affinity', 'view_affinity_steps', 'person_steps',
               'person_steps_labels', 'person_rays', 'smooth_tracks', 'associate_tracks-greedy', 'associate_tracks-optimal',
               'associate_tracks_rays', 'track_bone_lengths', 'predict_boxes']


@gpu
@pytest.mark.parametrize('name', HEADS_CALLS)
def test_heads_wrapper_on_a_side_stream(ctx, name):
    """A heads wrapper on device-resident inputs under torch.cuda.stream(s): no synchronisation (it returns while the delay in
    front of it runs), the bits of the call on the default stream."""
    a, b, fn = _heads_calls(ctx)[name]
    _chain(ctx, fn, a, b, f'heads.{name}', True)


def _rig_frames(ctx, which):
    rng = _rng(which, 'rig-frames')
    return [ctx.up(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)) for _ in range(6)]


def _frames_chains(ctx):
    """name -> fn(*six device frames): the frames calls on the rig of tests/test_gpu_world_follow.py (3 cameras x 2 exposures,
    two boxes on each frame), device-resident frames; device boxes where the call takes them."""
    from tests.test_gpu_world_follow import _rig
    path = ctx.model()[2]
    sk = ctx.model()[0].skeleton
    cams, _, boxes, fi, stamps = _rig()
    d_boxes, d_fi = ctx.up(boxes), ctx.up(fi.astype(np.int32))
    bones = np.random.default_rng(2).uniform(200, 450, len(sk.head_edges))
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, capacity=8)
    one = lambda f: list(f[:3])
    sel = fi < 3
    return {
        'estimate_pose_in_frames': lambda *f: FR.estimate_pose_in_frames(list(f), d_boxes, path, cameras=cams, frame_index=d_fi)[0],
        'locate_poses_in_frames-views': lambda *f: FR.locate_poses_in_frames(list(f), d_boxes, path, cameras=cams, frame_index=d_fi,
                                                                             bone_lengths=bones, views=2),
        'match_poses_in_frames': lambda *f: FR.match_poses_in_frames(one(f), boxes[sel], path, cams[:3], fi[sel], max_cost_mm=600.0),
        'follow_world_poses_in_frames': lambda *f: FR.follow_world_poses_in_frames(list(f), boxes, path, cams, fi, stamps, **kw),
        'follow_rig_poses_in_frames': lambda *f: FR.follow_rig_poses_in_frames(list(f), boxes, path, cams, fi, stamps, **kw),
        'Follower-camera': lambda *f: FR.Follower(path, cams[0], capacity=8, scale_recovery='true-root-depth',
                                                  root_depth=np.full(int(sel.sum()) // 3, 4000.0)).follow(list(f[:1]), boxes[fi == 0], fi[fi == 0], stamps[:1]),
        'Follower-world-learn_bones': lambda *f: FR.Follower(path, cams[:3], world=True, learn_bones=True, capacity=8, match_max_cost_mm=600.0,
                                                             max_cost_mm=590.0).follow(one(f), boxes[sel], fi[sel], stamps[:3]),
    }


FRAMES_CHAINS = ['estimate_pose_in_frames', 'locate_poses_in_frames-views', 'match_poses_in_frames', 'follow_world_poses_in_frames',
                 'follow_rig_poses_in_frames', 'Follower-camera', 'Follower-world-learn_bones']


@gpu
@pytest.mark.parametrize('name', FRAMES_CHAINS)
def test_frames_chain_on_a_side_stream(ctx, name):
    """A frames call under torch.cuda.stream(s) behind the delay, on frames that are copied into place on s: the bits of the same
    call on the default stream.  Each makes one documented host synchronisation (module docstring): ordering is proven for the
    launches in front of it."""
    fn = _frames_chains(ctx)[name]
    _chain(ctx, fn, _rig_frames(ctx, 'A'), _rig_frames(ctx, 'B'), f'frames.{name}', False)


@gpu
def test_estimate_pose_on_a_side_stream(ctx):
    from metro_pose3d_amd.inference import estimate_pose
    path = ctx.model()[2]
    _chain(ctx, lambda images: estimate_pose(images, path)[0], [ctx.images('A')], [ctx.images('B')], 'inference.estimate_pose', False)


@gpu
def test_metrics_and_warp_crops_on_a_side_stream(ctx):
    from metro_pose3d_amd.metrics import eval_metrics
    from metro_pose3d_amd.preprocess import box_homography, warp_crops
    pose = lambda which, tag: ctx.up(_rng(which, tag).normal(0, 300, (2, 17, 3)).astype(np.float32))

    def metrics(pred, true):
        m = eval_metrics(pred, true)
        return m['dist'], m['dist_procrustes'], torch.from_numpy(np.asarray([m['mean_error'], m['mean_error_procrustes'], m['mean_pck']])).to(ctx.dev)
    _chain(ctx, metrics, [pose('A', 'pred'), pose('A', 'true')], [pose('B', 'pred'), pose('B', 'true')], 'metrics.eval_metrics', False)
    homs = ctx.up(np.stack([box_homography(b, WARP_SIDE) for b in WARP_BOXES]))           # on the device: nothing to upload
    _chain(ctx, lambda frame: warp_crops(frame, homs, WARP_SIDE), [_frame(ctx, 'A')], [_frame(ctx, 'B')], 'preprocess.warp_crops', True)
