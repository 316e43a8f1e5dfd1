"""'Flagged, or right' on whole forwards (`-m gpu`): an fp16 overflow that begins at a few pixels of one channel, several units
in front of the head -- the way a real checkpoint overflows first.

The property, per crop of a call of three: status_words(3)[i] == 1, or the f16 pose is as close to the f64 engine's pose on the
same parameters and images as it is for a healthy model.  tests/test_gpu_forward.py:test_fp16_overflow_is_reported_not_returned
holds the screen on a net that overflows everywhere (every conv3 at 3x gain: fresh +Inf in every unit up to the head); here the
parameters are synth.make_params with the healthy logit gain and the default res_gain, and ONE doctoring at a time:

  stream   unit U, one output channel c of its conv3: its weights and bias are scaled by +-1.2 * 65504 / m, m = max |conv3 output
           of channel c| over the three crops (fp64, from the f64 engine's dump of U's conv2: the branch is what the weights
           scale; the shortcut's addend is not).  Only pixels within 1 / 1.2 of the channel's maximum overflow; 1.2 is a
           construction choice, not a measurement.  c is the channel whose two signs are the most lopsided, so that one of the
           two doctorings sends its extreme to -Inf and little else anywhere: the benign direction (relu(-Inf) = 0 is what the
           f64 engine computes from the hugely negative value too).  U: the last unit; the third-last unit of block4 (its
           projection-shortcut unit); the last unit of block3, in front of it; block1/unit_2.
  branch   the same for one conv1 output channel (t1) of block3/unit_3, through the folded BatchNorm's gamma and beta; t1 is
           stored behind a ReLU, so m is the maximum of the side that the sign turns positive.
  head     one logits bias is NaN, then +Inf: every crop must be flagged; then -Inf (a voxel of weight zero): flagged or right.

Each stream / branch doctoring asserts on the f16 engine's dump of the doctored layer that at least one and at most 5 % of its
elements are non-finite: a condition the construction satisfies, so that no case passes by never overflowing, nor by overflowing
everywhere.  test_the_screen_is_exercised asserts that some doctoring produced a flagged crop, some an unflagged crop that agrees
with f64; every case asserts first that its healthy model has status 0 for every crop.

The bound.  d0 = the largest |f16 - f64| (mm) over the crops of the healthy model, computed here.  A crop that is not flagged must
be within K * d0.  K was not fixed in advance: the doctorings were run once on the parent commit's kernels (maxNum ReLUs) and on
these, and K lies between the two figures below.

Measured on an MI355X (d0: toy-s32 2.131, toy-s16-many19 2.244, toy-s32-side224 2.365, rn50-s32 3.030 mm):
  * the largest distance of an unflagged crop in a benign case (an extreme sent to -Inf, a relu(-Inf) = 0 downstream): 1.04 x d0
    (2.220 mm on toy-s32, 3.162 mm on rn50-s32) -- with the parent's kernels and with these, to the digit;
  * the smallest distance of a case that is wrong: 771 x d0.  With the parent's maxNum ReLUs the doctoring toy-s32 / branch / plus
    (+Inf at 0.1 % of t1 in block3/unit_3) returned crops 0 and 1 UNFLAGGED, 1642.6 mm and 2737.7 mm from the f64 engine: conv2
    and conv3 sum infinities of both signs into NaN, the next prologues' max(NaN, 0) = 0 erase it, block4's projection shortcut
    reads only the pre-activated stream.  With metro::relu all three crops are flagged.
  K = 28 is the geometric middle of 1.04 and 771: almost three decades apart.
The stream doctorings at the third-last unit of block4 and the last unit of block3 pass on the parent's kernels as well: a +-Inf in
the stream itself is carried by the identity shortcuts and a +Inf passes a maxNum ReLU; it is the NaN born inside a branch that
the parent lost.  Every flagged case above is flagged by both.
The head plant -Inf holds softargmax_partial (the f64 engine, and the two-launch f16 path of toy-s32-side224) to treating a
channel that holds nothing but -Inf as weight zero: its running maximum starts at -Inf, and exponents taken about that maximum
would be exp(-Inf - -Inf) = NaN, so it takes them about 0.  The one-launch head gives such voxels weight zero as well; all nine
crops are unflagged and within 1.0 x d0 of the f64 engine.
"""
import functools

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, synth
from metro_pose3d_amd.engine import Engine, _bn_scale_shift
from tests.test_gpu_forward import TOY

pytestmark = pytest.mark.gpu

N = 3
F16_MAX = 65504.0
OVER = 1.2
K = 28.0

SPECS = {'toy-s32': TOY[0], 'toy-s16-many19': TOY[1], 'toy-s32-side224': ModelSpec(50, 32, 'h36m', base_width=8, proc_side=224),
         'rn50-s32': ModelSpec(50, 32, 'h36m')}
STREAM_UNITS = {'last': 'block4/unit_3', 'block4-third-last': 'block4/unit_1', 'block3-last': 'block3/unit_6', 'block1-unit2': 'block1/unit_2'}
BRANCH_UNIT, BRANCH_INPUT = 'block3/unit_3', 'block3/unit_2'
_SIGN = {1: 'plus', -1: 'minus'}

# (model, kind, where, sign or value)
DOCTORINGS = [(m, 'stream', u, s) for m in ('toy-s32', 'toy-s16-many19', 'toy-s32-side224') for u in STREAM_UNITS for s in (1, -1)] + \
    [(m, 'branch', BRANCH_UNIT, s) for m in ('toy-s32', 'toy-s16-many19', 'toy-s32-side224') for s in (1, -1)] + \
    [(m, 'head', 'logits-bias', v) for m in ('toy-s32', 'toy-s16-many19', 'toy-s32-side224') for v in ('nan', '+inf', '-inf')] + \
    [('rn50-s32', 'stream', u, s) for u in ('block4-third-last', 'block3-last') for s in (1, -1)]      # the f64 engine at real width is the cost
_doc_id = lambda d: f'{d[0]}-{d[1]}-{d[2]}-{_SIGN.get(d[3], d[3])}'


class _Model:
    """One spec: its healthy parameters, three crops, one f16 and one f64 engine (re-bound per doctoring), the healthy distance."""

    def __init__(self, key, cuda):
        self.spec = spec = SPECS[key]
        self.root = f'MainPart/resnet_v2_{spec.arch}'
        self.params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                                        logit_gain=synth.logit_gain_for(spec.arch, spec.stride, spec.base_width))
        self.images = torch.from_numpy(synth.make_images(N, spec.proc_side)).to(cuda)
        self.cuda = cuda
        self.e16 = Engine(spec, self.params, 'f16', max_batch=N, device=cuda)
        self.e64 = Engine(spec, self.params, 'f64', max_batch=N, device=cuda)
        self.names16 = [li.name.decode() for li in self.e16.layer_infos()]
        self.names64 = [li.name.decode() for li in self.e64.layer_infos()]
        self.bound = self.params
        flagged, dist = self.run()
        self.healthy_flagged, self.d0 = flagged, float(dist.max())

    def use(self, params):
        if self.bound is not params:
            torch.cuda.synchronize()            # queued launches still read the blob the engines are about to replace
            self.e16.bind(params, self.cuda)
            self.e64.bind(params, self.cuda)
            self.bound = params

    def run(self):
        """(flagged [N] bool, |f16 - f64| per crop in mm: inf where either pose is not finite) of the bound parameters."""
        p16 = self.e16.forward(self.images)
        flagged = self.e16.status_words(N).cpu().numpy() != 0
        p16 = p16.cpu().double().numpy()
        p64 = self.e64.forward(self.images).cpu().double().numpy()
        with np.errstate(invalid='ignore'):
            dist = np.abs(p16 - p64).reshape(N, -1).max(axis=1)
        dist[~np.isfinite(p16).reshape(N, -1).all(axis=1) | ~np.isfinite(p64).reshape(N, -1).all(axis=1)] = np.inf
        return flagged, dist

    def dump64(self, name):
        self.use(self.params)
        return self.e64.forward_upto(self.images, self.names64.index(name)).cpu().double().numpy()

    def dump16(self, prefix):
        i = next(i for i, nm in enumerate(self.names16) if nm == prefix or nm.startswith(prefix + '+'))
        return self.e16.forward_upto(self.images, i).float().cpu().numpy()

    # ---- the doctorings: -> (parameters, layer of the f16 plan whose dump must hold the overflow, or None) ----
    def stream(self, unit, sign):
        scope = f'{self.root}/{unit}/bottleneck_v2/conv3'
        w, b = self.params[scope + '/weights'], self.params[scope + '/biases']
        branch = self.dump64(f'{unit}/conv2') @ w[0, 0].astype(np.float64) + b.astype(np.float64)        # conv3 has no BatchNorm
        hi, lo = branch.max(axis=(0, 1, 2)), -branch.min(axis=(0, 1, 2))
        c = int(np.argmax(np.maximum(hi, lo) / np.maximum(np.minimum(hi, lo), 1e-30)))
        g = sign * OVER * F16_MAX / max(hi[c], lo[c])
        p = dict(self.params)
        p[scope + '/weights'], p[scope + '/biases'] = w.copy(), b.copy()
        p[scope + '/weights'][..., c] *= g
        p[scope + '/biases'][c] *= g
        return p, f'{unit}/conv3'

    def branch(self, unit, sign):
        scope = f'{self.root}/{unit}/bottleneck_v2'
        ps, pb = _bn_scale_shift(self.params, scope + '/preact')
        sc, sh = _bn_scale_shift(self.params, scope + '/conv1/BatchNorm')
        x = np.maximum(self.dump64(f'{BRANCH_INPUT}/conv3') * ps + pb, 0.0)
        v = sign * (x @ (self.params[scope + '/conv1/weights'][0, 0].astype(np.float64) * sc) + sh)       # conv1 in front of its ReLU
        top = v.max(axis=(0, 1, 2))
        c = int(np.argmax(top))
        g = sign * OVER * F16_MAX / top[c]
        p = dict(self.params)
        for k in ('/conv1/BatchNorm/gamma', '/conv1/BatchNorm/beta'):             # folded scale and shift, both times g
            p[scope + k] = self.params[scope + k].copy()
            p[scope + k][c] *= g
        return p, f'{unit}/conv1'

    def head(self, _where, value):
        p = dict(self.params)
        p[self.root + '/logits/biases'] = self.params[self.root + '/logits/biases'].copy()
        p[self.root + '/logits/biases'][0] = float(value)
        return p, None


@functools.lru_cache(maxsize=None)
def _model(key, cuda):
    return _Model(key, cuda)


@functools.lru_cache(maxsize=None)
def outcome(doc, cuda):
    """(flagged [N], distance [N] in mm, d0, share of non-finite elements in the doctored layer's f16 dump or None)."""
    key, kind, where, arg = doc
    m = _model(key, cuda)
    params, layer = getattr(m, kind)(STREAM_UNITS.get(where, where), arg)
    m.use(params)
    share = None if layer is None else float((~np.isfinite(m.dump16(layer))).mean())
    flagged, dist = m.run()
    print(f'{_doc_id(doc)}: d0 {m.d0:.3f} mm  flagged {flagged.astype(int).tolist()}  |f16 - f64| {np.round(dist, 3).tolist()} mm  '
          f'non-finite share of the doctored layer {share}')
    return flagged, dist, m.d0, share


@pytest.mark.parametrize('doc', DOCTORINGS, ids=_doc_id)
def test_flagged_or_right(cuda, doc):
    flagged, dist, d0, share = outcome(doc, cuda)
    healthy = _model(doc[0], cuda).healthy_flagged
    assert not healthy.any() and np.isfinite(d0) and d0 > 0, f'{doc[0]}: the healthy model is flagged {healthy.tolist()}, d0 = {d0}'
    if share is not None:
        assert 0.0 < share <= 0.05, f'{_doc_id(doc)}: {share:.2%} of the doctored layer is non-finite in f16 (the construction wants 0 < share <= 5 %)'
    if doc[1] == 'head' and doc[3] in ('nan', '+inf'):
        assert flagged.all(), f'{_doc_id(doc)}: a {doc[3]} logits bias reaches every crop, flagged {flagged.tolist()}'
    wrong = ~flagged & ~(dist <= K * d0)
    assert not wrong.any(), (f'{_doc_id(doc)}: crops {np.flatnonzero(wrong).tolist()} are not flagged and {dist[wrong].tolist()} mm from the '
                             f'f64 engine (healthy distance d0 = {d0:.3f} mm, bound {K} x d0)')


def test_the_screen_is_exercised(cuda):
    """Without these the file is vacuous: a healthy model is never flagged, some doctoring is flagged, and some doctoring leaves a
    crop unflagged that agrees with f64 (the benign -Inf direction)."""
    docs = [d for d in DOCTORINGS if d[0] == 'toy-s32']
    m = _model('toy-s32', cuda)
    assert not m.healthy_flagged.any() and np.isfinite(m.d0) and m.d0 > 0, (m.healthy_flagged, m.d0)
    results = [outcome(d, cuda) for d in docs]
    assert any(f.any() for f, _, _, _ in results), 'no doctoring produced a flagged crop'
    assert any((~f & (dist <= K * d0)).any() for f, dist, d0, _ in results), 'no doctoring left an unflagged crop that agrees with f64'
