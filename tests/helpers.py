"""Shared test plumbing: calling the C ABI with torch device buffers, oracle-side references."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')


def compile_for_host(tmp, name, sources, body) -> C.CDLL:
    """The __host__ __device__ code of the csrc files `sources`, compiled for the host: `tmp`/`name`.hip includes them in
    order, `body` (extern "C" wrappers around their functions) follows, and the shared object is opened.  The launchers in the
    sources link against the library's helpers, so the library is loaded first."""
    src = tmp / f'{name}.hip'
    src.write_text(''.join(f'#include "{os.path.join(CSRC, f)}"\n' for f in sources) + body)
    from metro_pose3d_amd.build import _hipcc
    so = tmp / f'{name}.so'
    pkg = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([_hipcc(), '--offload-arch=gfx950', '-O2', '-std=c++17', '-fPIC', '-shared', '-x', 'hip', str(src),
                           '-o', str(so), '-L' + pkg, '-l:' + os.path.basename(_lib.LIB_PATH), '-Wl,-rpath,' + pkg])
    _lib.load()
    return C.CDLL(str(so))


def conv_desc(n, h_in, c_in, h_out, c_out, k, stride=1, dil=1, pad=0, prologue=False, relu=False,
              residual=False, res_h=0, res_stride=1, res_offset=0, out_dtype=_lib.METRO_F16,
              w_in=None, w_out=None, in_pix_stride=None, kh=None, kw=None, in_dtype=None,
              pad_top=None, pad_left=None, res_w=None):
    d = _lib.MetroConvDesc()
    d.n = n
    d.h_in = h_in
    d.w_in = w_in if w_in is not None else h_in
    d.c_in = c_in
    d.in_pix_stride = in_pix_stride if in_pix_stride is not None else c_in
    d.h_out = h_out
    d.w_out = w_out if w_out is not None else h_out
    d.c_out = c_out
    d.kh = kh if kh is not None else k
    d.kw = kw if kw is not None else k
    d.stride = stride
    d.dilation = dil
    d.pad_top = d.pad_left = pad
    if pad_top is not None:
        d.pad_top = pad_top
    if pad_left is not None:
        d.pad_left = pad_left
    d.has_prologue = int(prologue)
    d.relu = int(relu)
    d.has_residual = int(residual)
    d.res_h = res_h
    d.res_w = res_w if res_w is not None else res_h
    d.res_stride = res_stride
    d.res_offset = res_offset
    d.out_dtype = out_dtype
    d.in_dtype = in_dtype if in_dtype is not None else (
        _lib.METRO_F16 if out_dtype == _lib.METRO_F16 else out_dtype)
    return d


def ref_conv_nhwc(x, w_ok, bias, stride, dil, pad, h_out, pro=None, relu=False, res=None,
                  res_stride=1, res_offset=0):
    """fp64 reference of one MetroConvDesc: x [N,H,W,C], w_ok [O, kh, kw, C] (the packed layout).

    `pad` is (pad_top == pad_left); the bottom/right pad is whatever makes the output h_out wide,
    i.e. taps that fall outside read zeros (TF zero padding, reference resnet_utils.py:125-135)."""
    x = torch.as_tensor(x, dtype=torch.float64)
    w = torch.as_tensor(w_ok, dtype=torch.float64)
    if pro is not None:
        sc, sh = (torch.as_tensor(t, dtype=torch.float64) for t in pro)
        x = torch.relu(x * sc + sh)
    n, h, wd, c = x.shape
    o, kh, kw, _ = w.shape
    need_h = (h_out - 1) * stride + (kh - 1) * dil + 1
    need_w = (h_out - 1) * stride + (kw - 1) * dil + 1
    # tap (r,s) of output (ho,wo) reads input (ho*stride - pad + r*dil, ...), zero outside
    big = max(pad, 0)
    xp = torch.zeros((n, big + max(h, need_h - pad) + 1, big + max(wd, need_w - pad) + 1, c),
                     dtype=torch.float64)
    xp[:, big:big + h, big:big + wd] = x
    xp = xp[:, big - pad:big - pad + need_h, big - pad:big - pad + need_w]
    y = torch.nn.functional.conv2d(xp.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, stride=stride,
                                   dilation=dil).permute(0, 2, 3, 1)
    y = y + torch.as_tensor(bias, dtype=torch.float64)
    if relu:
        y = torch.relu(y)
    if res is not None:
        r = torch.as_tensor(res, dtype=torch.float64)
        y = y + r[:, res_offset::res_stride, res_offset::res_stride][:, :h_out, :h_out]
    return y


def ref_conv_desc(d, x, w_ok, bias, pro=None, pro_round=np.float16, res=None):
    """fp64 tap-sum restatement of one MetroConvDesc `d`, for any geometry the descriptor can state.

    x: [n, h_in, w_in, P] with P >= d.c_in -- the input pixels as the kernel sees them (P = d.in_pix_stride for a strided
    buffer); channels [0, c_in) are read.  w_ok [c_out, kh, kw, c_in] (the packed layout), bias [c_out].
    Tap (r, s) of output (ho, wo) reads input row ho*stride - pad_top + r*dilation, column wo*stride - pad_left + s*dilation;
    a tap outside the input reads zero.  pro = (scale, shift): the input becomes relu(x*scale + shift), rounded ONCE to
    `pro_round` (fp16 for the fp16 kernels; None = kept in fp64).  Then bias, ReLU (if d.relu) and the residual
    res [n, res_h, res_w, c_out] at pixel (ho*res_stride + res_offset, wo*res_stride + res_offset).

    Returns (y, a): y the exact result, a = sum|w*x| + |bias| (+ |res|), the absolute condition sum of every output element
    (what bounds the error of any summation order of the same terms)."""
    c_in = d.c_in
    x = np.asarray(x, dtype=np.float64)[..., :c_in]
    assert x.shape == (d.n, d.h_in, d.w_in, c_in), (x.shape, (d.n, d.h_in, d.w_in, c_in))
    w = np.asarray(w_ok, dtype=np.float64)
    assert w.shape == (d.c_out, d.kh, d.kw, c_in), w.shape
    if pro is not None:
        x = x * np.asarray(pro[0], np.float64) + np.asarray(pro[1], np.float64)
        if pro_round is not None:
            x = x.astype(pro_round).astype(np.float64)
        x = np.maximum(x, 0.0)
    ho = np.arange(d.h_out) * d.stride - d.pad_top
    wo = np.arange(d.w_out) * d.stride - d.pad_left
    y = np.zeros((d.n, d.h_out, d.w_out, d.c_out))
    a = np.zeros_like(y)
    for r in range(d.kh):
        rows = ho + r * d.dilation
        rok = (rows >= 0) & (rows < d.h_in)
        for s in range(d.kw):
            cols = wo + s * d.dilation
            cok = (cols >= 0) & (cols < d.w_in)
            xt = x[:, np.clip(rows, 0, d.h_in - 1)][:, :, np.clip(cols, 0, d.w_in - 1)]
            # (a select, not a product: a tap outside the input reads zero even where the clipped gather found Inf or NaN)
            xt = np.where((rok[:, None] & cok[None, :])[None, :, :, None], xt, 0.0)
            wt = w[:, r, s, :].T
            y += xt @ wt
            a += np.abs(xt) @ np.abs(wt)
    b = np.asarray(bias, np.float64)
    y += b
    a += np.abs(b)
    if d.relu:
        y = np.maximum(y, 0.0)
    if d.has_residual:
        rr = np.arange(d.h_out) * d.res_stride + d.res_offset
        rc = np.arange(d.w_out) * d.res_stride + d.res_offset
        rg = np.asarray(res, np.float64)[:, rr][:, :, rc]
        y += rg
        a += np.abs(rg)
    return y, a


DYADIC_SCALES = (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5)


def dyadic_conv_operands(rng, d, lim=8):
    """Operands of MetroConvDesc `d` on which ANY summation order of a conv kernel with fp32 (or wider) accumulators gives the
    exact result: inputs and weights integers / 8 in [-lim / 8, lim / 8], bias and residual integers / 64 in [-1, 1], prologue
    scales from DYADIC_SCALES (negative and zero folded BN scales included), shifts integers / 8 in [-1, 1] -- every product is
    a multiple of 2^-6 (2^-8 behind a prologue), so every partial sum is exact while it stays below 2^24 of that unit
    (exact_sum_condition).  fp64 arrays (x, w, bias, pro or None, res or None); every value is exact in fp16 too."""
    ints = lambda shape, m, q: rng.integers(-m, m + 1, shape).astype(np.float64) / q
    x = ints((d.n, d.h_in, d.w_in, d.c_in), lim, 8)
    w = ints((d.c_out, d.kh, d.kw, d.c_in), lim, 8)
    b = ints(d.c_out, 64, 64)
    pro = (rng.choice(DYADIC_SCALES, d.c_in), ints(d.c_in, 8, 8)) if d.has_prologue else None
    res = ints((d.n, d.res_h, d.res_w, d.c_out), 64, 64) if d.has_residual else None
    return x, w, b, pro, res


def exact_sum_condition(a, prologue):
    """Whether every partial sum of every output element is exact in fp32 on dyadic_conv_operands: a * 2^f < 2^24 for the
    condition sums `a` of ref_conv_desc, f = the fractional bits of a product (6; 8 behind a prologue)."""
    return bool((np.asarray(a) * 2.0 ** (8 if prologue else 6) < 2.0 ** 24).all())


def run_conv_f16(lib, dev, d, x, w, bias, pro=None, res=None):
    """x, w, pro, res: numpy (cast to fp16); bias fp32.  Returns numpy of d.out_dtype."""
    tx = torch.from_numpy(np.ascontiguousarray(x.astype(np.float16))).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(w.astype(np.float16))).to(dev)
    tb = torch.from_numpy(np.ascontiguousarray(bias.astype(np.float32))).to(dev)
    ts = tsh = tr = None
    if pro is not None:
        ts = torch.from_numpy(pro[0].astype(np.float16)).to(dev)
        tsh = torch.from_numpy(pro[1].astype(np.float16)).to(dev)
    if res is not None:
        tr = torch.from_numpy(np.ascontiguousarray(res.astype(np.float16))).to(dev)
    odt = torch.float16 if d.out_dtype == _lib.METRO_F16 else torch.float32
    out = torch.full((d.n, d.h_out, d.w_out, d.c_out), float('nan'), dtype=odt, device=dev)
    check(lib.metro_conv_f16(C.byref(d), ptr(tx), ptr(tw), ptr(tb), ptr(ts), ptr(tsh), ptr(tr), ptr(out),
                             C.c_void_p(0)), 'metro_conv_f16')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_conv_f64acc(lib, dev, d, x, w, bias, pro=None, res=None):
    np_in = np.float32 if d.in_dtype == _lib.METRO_F32 else np.float64
    np_out = np.float32 if d.out_dtype == _lib.METRO_F32 else np.float64
    tx = torch.from_numpy(np.ascontiguousarray(x.astype(np_in))).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(w.astype(np.float64))).to(dev)
    tb = torch.from_numpy(np.ascontiguousarray(bias.astype(np.float64))).to(dev)
    ts = tsh = tr = None
    if pro is not None:
        ts = torch.from_numpy(pro[0].astype(np.float64)).to(dev)
        tsh = torch.from_numpy(pro[1].astype(np.float64)).to(dev)
    if res is not None:
        tr = torch.from_numpy(np.ascontiguousarray(res.astype(np_out))).to(dev)
    out = torch.full((d.n, d.h_out, d.w_out, d.c_out), float('nan'),
                     dtype=torch.float32 if np_out is np.float32 else torch.float64, device=dev)
    check(lib.metro_conv_f64acc(C.byref(d), ptr(tx), ptr(tw), ptr(tb), ptr(ts), ptr(tsh), ptr(tr),
                                ptr(out), C.c_void_p(0)), 'metro_conv_f64acc')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_softargmax(lib, dev, spec, logits, precise):
    """spec: metro_pose3d_amd.ModelSpec; logits numpy [n,S,S,D*J] fp32."""
    n = logits.shape[0]
    cs = spec.to_c(int(precise))
    tl = torch.from_numpy(np.ascontiguousarray(logits.astype(np.float64 if int(precise) == 2 else np.float32))).to(dev)
    sb = lib.metro_softargmax_scratch_bytes(n, spec.heatmap_side, spec.skeleton.n_head)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    out = torch.full((n, spec.skeleton.n_out, 3), float('nan'), dtype=torch.float32, device=dev)
    check(lib.metro_softargmax(ptr(tl), n, C.byref(cs), int(precise), ptr(scratch), ptr(out),
                               C.c_void_p(0)), 'metro_softargmax')
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- batches of twins: a call of n crops built from p oracle-checked images, every position held through its twin ------------------

TWIN_GROUPS = (2, 4, 8, 16)     # images per tile / per block round the kernels walk in: aligned groups of these sizes


def _assignment_faults(a, p):
    """What keeps `a` from being a crop assignment (crop_assignment's conditions); None if nothing does."""
    n = len(a)
    if not np.array_equal(a[:p], np.arange(p)) or a[n - 1] != p - 1:
        return 'the first p positions are not 0..p-1, or the last is not p - 1'
    for s in range(1, n):
        if np.array_equal(a[:n - s], a[s:]):
            return f'a shift by {s} images maps the sequence onto itself'
    for g in TWIN_GROUPS:
        groups = a[:n // g * g].reshape(-1, g)
        same = np.flatnonzero((groups[:-1] == groups[1:]).all(axis=1)) if 2 * g <= n else []
        if len(same):
            return f'the aligned groups of {g} images at {same[0] * g} and {(same[0] + 1) * g} have the same pattern'
    at = np.arange(n)
    for s in range(1, n):                   # out[i] = table[a[(i + s) % n]]: the twin check sees it iff out[i] != out[a[i]] somewhere
        if np.array_equal(a[(at + s) % n], a[(a + s) % n]):
            return f'a rotation of the batch by {s} images passes the twin check'
    return None


def crop_assignment(n, p, seed):
    """int64 [n]: position i of a call of n crops holds base image assign[i] of p -- the layout of a batch whose first p
    positions are compared with an oracle and whose other positions must carry the bits of their twin (assert_twins).

    Unlike `i % p` the sequence has no symmetry a misplaced tile could hide behind (each is asserted here):
      * assign[:p] is 0..p-1 and, for n > p, assign[n-1] == p - 1: the first and the last position of the call are anchored to
        different oracle-checked images, and every base image occurs;
      * no shift maps the sequence onto itself: for every s in 1..n-1 some assign[i] != assign[i + s];
      * for g in 2, 4, 8, 16 with 2 g <= n no two adjacent aligned groups of g images have the same pattern, so a swap of two
        such groups (two blocks exchanging tiles, a tile stored into the next tile's slot) always moves some image onto a
        different one.  g = 1 cannot be had: with n > p some neighbours are equal, and a swap of two equal neighbours changes
        nothing in the inputs either -- it is undetectable by construction;
      * no rotation of the batch by 1..n-1 images passes assert_twins on its own (a rotated output whose first p positions still
        look like p distinct images to the gather).
    n <= p gives the identity.  Deterministic: the middle is drawn from np.random.default_rng([seed, n, p]), an element that
    would complete a repeated group is redrawn among the values that do not (with none left, the 16 positions in front are drawn
    again), and the seed is stepped until everything holds (n > p needs p >= 2)."""
    if n <= p:
        return np.arange(n)
    if p < 2:
        raise ValueError('a batch of twins needs at least two base images')
    for step in range(1000):
        rng = np.random.default_rng([seed + step, n, p])
        a = rng.integers(0, p, n)
        a[:p] = np.arange(p)
        a[n - 1] = p - 1
        i, redraws = p, 0
        while i < n and redraws < 100:
            # the values that would make the aligned group ending at i a copy of the group in front of it
            bad = {a[i - g] for g in TWIN_GROUPS if (i + 1) % g == 0 and i + 1 >= 2 * g and np.array_equal(a[i - g + 1:i], a[i - 2 * g + 1:i - g])}
            free = [v for v in ([p - 1] if i == n - 1 else range(p)) if v not in bad]
            if a[i] in free:
                i += 1
            elif free:
                a[i] = free[rng.integers(len(free))]
                i += 1
            else:                                   # no value is left (p = 2): draw the last 16 positions again
                back = max(p, i - 16)
                a[back:min(i + 1, n - 1)] = rng.integers(0, p, min(i + 1, n - 1) - back)
                i, redraws = back, redraws + 1
        if i == n and _assignment_faults(a, p) is None:
            break
    fault = _assignment_faults(a, p)
    assert fault is None, f'crop_assignment({n}, {p}, {seed}): {fault}'
    return a


TWIN_CHUNK_ELEMENTS = 2 ** 28  # lay_out_twins / assert_twins gather and compare at most this many elements at a time (whole images)


def _image_groups(n, per_image, chunk):
    """(start, stop) runs of whole images with at most `chunk` elements each (one image where an image alone has more)."""
    step = max(1, chunk // max(1, per_image))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def lay_out_twins(base, assign, chunk=TWIN_CHUNK_ELEMENTS):
    """The batch base[assign]: [n, ...] from the p base images, a device tensor or a numpy array like `base`.  A device batch of
    more than `chunk` elements is gathered in groups of whole images: no single gather spans 2^31 elements."""
    if isinstance(base, np.ndarray):
        return np.ascontiguousarray(base[assign])
    idx = torch.as_tensor(assign, device=base.device)
    per = base[0].numel()
    if len(assign) * per <= chunk:
        return base[idx].contiguous()
    out = torch.empty((len(assign),) + tuple(base.shape[1:]), dtype=base.dtype, device=base.device)
    for i, j in _image_groups(len(assign), per, chunk):
        out[i:j] = base[idx[i:j]]
    return out


def assert_twins(out, assign, p, what, chunk=TWIN_CHUNK_ELEMENTS):
    """Every position of `out` [n, ...] carries the bits of its base image's first occurrence: out == out[:p][assign], gathered
    on out's device (on the bit patterns of float tensors: NaN equals NaN).  A tensor of more than `chunk` elements is gathered
    and compared in groups of whole images -- the same comparison of every element and the same message, the first position that
    differs -- so neither the copy nor the compare spans 2^31 elements (tensors beyond 4 GiB: tests/test_gpu_large_address.py)."""
    assert out.shape[0] == len(assign), (what, out.shape, len(assign))
    if out.is_floating_point():
        out = out.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[out.element_size()])
    idx = torch.as_tensor(assign, device=out.device)
    for lo, hi in _image_groups(len(assign), out[0].numel(), max(chunk, 1)):
        part = out[lo:hi]
        want = out[:p][idx[lo:hi]]
        if torch.equal(part, want):
            continue
        i = lo + int((part != want).reshape(hi - lo, -1).any(dim=1).nonzero()[0])
        raise AssertionError(f'{what}: position {i} of {len(assign)} differs from its twin, position {int(assign[i])} (base image {int(assign[i])})')


def wrap_assignment(n, p, seed, wraps):
    """crop_assignment(n, p, seed') with the seed stepped until, for every (first, distance) of `wraps`, some position
    i >= first holds a different base image than position i - distance.  `first` is the first image that lies wholly beyond an
    address boundary (2^31 or 2^32 bytes, 2^31 elements), `distance` the boundary in images: an access whose address wraps at the
    boundary lands `distance` images lower, on ANOTHER image -- a wrapped load reads the wrong image, a wrapped store leaves NaN
    above or overwrites a different image below.  crop_assignment itself promises only that some position differs per shift,
    not one beyond `first`.  -> (assignment, seed used)."""
    for step in range(1000):
        a = crop_assignment(n, p, seed + step)
        if all(d <= first < n and (a[first:] != a[first - d:n - d]).any() for first, d in wraps):
            return a, seed + step
    raise AssertionError(f'wrap_assignment({n}, {p}, {seed}, {wraps}): no seed gives every wrap a differing pair')


def oracle_spec(spec):
    """metro_pose3d_amd.ModelSpec -> oracle.spec.OracleSpec (same field names by design)."""
    from oracle.spec import OracleSpec
    return OracleSpec(arch=spec.arch, stride=spec.stride, dataset=spec.dataset, depth=spec.depth,
                      centered_stride=spec.centered_stride, proc_side=spec.proc_side,
                      box_size_mm=spec.box_size_mm, base_width=spec.base_width)


def assert_as_accurate_as_fp16_model(spec, params, images, poses, what='', ratio_mean=2.0, ratio_max=2.5):
    """The accuracy criterion of the f16 mode: `poses` (the HIP path's, for exactly these crops) may
    not be further from exact math (fp64 oracle) than the one-rounding-per-tensor fp16 model of the graph (oracle/f16emu.py)
    is itself -- mean within ratio_mean, maximum within ratio_max (two draws of the same rounding noise)."""
    from oracle import f16emu
    from oracle import forward as OF
    ospec = oracle_spec(spec)
    exact = OF.forward(ospec, params, images, torch.float64).numpy()
    emu = f16emu.forward(ospec, params, images).numpy()
    poses = np.asarray(poses, dtype=np.float64)
    assert np.isfinite(poses).all(), what
    d, de = np.abs(poses - exact), np.abs(emu - exact)
    assert d.mean() <= ratio_mean * de.mean() and d.max() <= ratio_max * de.max(), \
        f'{what}: |hip - fp64| mean {d.mean():.3f} max {d.max():.3f} mm vs the fp16 model\'s own {de.mean():.3f} / {de.max():.3f} mm'
    return float(d.max()), float(de.max())


# ---- the bone-length z-offset solve: the problems its kernels are tested on, and their scipy reference -----------------

BONE_FAMILIES = ('friendly', 'noisy', 'mis-scaled', 'collapsed')


def bone_spec(dataset):
    """One model per skeleton for the bone-length corpus (stride, centring and crop side differ on purpose)."""
    from metro_pose3d_amd import ModelSpec
    return {'h36m': ModelSpec(50, 16, 'h36m'), 'many19': ModelSpec(50, 8, 'many19', proc_side=384),
            'merged': ModelSpec(50, 32, 'merged', centered_stride=False, proc_side=224)}[dataset]


def consistent_problem(rng, spec, n):
    """Synthetic but geometrically consistent inputs: coords01 such that rays * depth reproduce a pose.
    -> (joint info, poses [n, J, 3], coords01 fp32 [n, J, 3], inv_k fp32 [n, 3, 3], true bone lengths [n, E])."""
    from oracle.spec import head_joint_info
    ji = head_joint_info(spec.dataset)
    j = ji.n_joints
    p = rng.normal(0, 300, (n, j, 3))
    p[..., 2] += rng.uniform(1500, 6000, (n, 1))
    f = rng.uniform(900, 1400, n)
    kk = np.zeros((n, 3, 3)); kk[:, 0, 0] = f; kk[:, 1, 1] = f; kk[:, 0, 2] = 128; kk[:, 1, 2] = 128; kk[:, 2, 2] = 1
    uv = np.einsum('nij,ncj->nci', kk, p / p[..., 2:3])[..., :2]
    last = spec.proc_side - 1
    lrc = last - (last % spec.stride) - 1
    c01 = np.empty((n, j, 3), np.float32)
    c01[..., :2] = ((uv - (spec.stride // 2 if spec.centered_stride else 0)) / lrc).astype(np.float32)
    c01[..., 2] = ((p[..., 2] - p[:, -1:, 2]) / 2200.0 + 0.5 + rng.normal(0, 0.01, (n, j))).astype(np.float32)
    inv_k = np.linalg.inv(kk).astype(np.float32)
    bones = np.array([[np.linalg.norm(p[i, a] - p[i, b]) for a, b in ji.edges] for i in range(n)])
    return ji, p, c01, inv_k, bones


def bone_problem(spec, family, n, seed=0):
    """n seeded z-offset problems of one family -> (joint info, coords01 fp32 [n, J, 3], inv_k fp32 [n, 3, 3],
    shared targets [E], per-pose targets [n, E]).
      friendly    a consistent pose; targets: its bones (per pose), their mean * 0.97 (shared)
      noisy       coords01 uniform in [0, 1]: no pose has these rays and depths; targets shrunk (* 10^U(-1.3, 0) per pose,
                  * 0.1 shared), which is where MINPACK's step control works longest, up to maxfev
      mis-scaled  a consistent pose, targets * 10^U(-1.3, 1.3): one factor per pose (per pose: the fitted depth is that
                  many times the true one) and one per bone (shared: no depth fits)
      collapsed   every joint at 0.5 +- N(0, 1e-4): edge vectors of ~1e-4 of the crop"""
    rng = np.random.default_rng([seed, BONE_FAMILIES.index(family), spec.skeleton.n_head])
    ji, _, c01, inv_k, bones = consistent_problem(rng, spec, n)
    shared, per_pose = bones.mean(axis=0) * 0.97, bones.copy()
    if family == 'noisy':
        c01 = rng.uniform(0, 1, c01.shape).astype(np.float32)
        per_pose = bones * 10 ** rng.uniform(-1.3, 0.0, (n, 1))
        shared = bones.mean(axis=0) * 0.1
    elif family == 'mis-scaled':
        per_pose = bones * 10 ** rng.uniform(-1.3, 1.3, (n, 1))
        shared = bones.mean(axis=0) * 10 ** rng.uniform(-1.3, 1.3, bones.shape[1])
    elif family == 'collapsed':
        c01 = (0.5 + rng.normal(0, 1e-4, c01.shape)).astype(np.float32)
    elif family != 'friendly':
        raise ValueError(family)
    return ji, c01, inv_k, shared, per_pose


def ulp32(x):
    """The spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


class BoneCase:
    """One (skeleton, family, target kind) of the corpus with its reference.
    z: scipy's solution on the oracle's fp32 coefficients, fp64 [n] (NaN where scipy refuses the problem);
    moved: the farthest that solution moves (mm) when every coefficient c, d, e goes one float32 ulp up, down, or in one of
    two seeded random sign patterns -- the oracle's own sensitivity to the last bit of what the kernel forms in fp32."""

    def __init__(self, dataset, family, per_pose, n=130, seed=0):
        from oracle import heads as OH
        self.spec = spec = bone_spec(dataset)
        self.family, self.per_pose, self.n = family, per_pose, n
        self.ji, self.c01, self.inv_k, shared, each = bone_problem(spec, family, n, seed)
        self.targets = each if per_pose else shared
        self.cam, self.dz = OH.camcoords_and_delta_z(self.c01, self.inv_k, spec.stride, spec.proc_side, spec.centered_stride,
                                                     spec.box_size_mm)
        rng = np.random.default_rng([seed, 77])
        self.z, self.moved = np.empty(n), np.zeros(n)
        for i in range(n):
            cde = OH.edge_coefficients(self.cam[i], self.dz[i], self.ji.edges)
            t = self.targets[i] if per_pose else self.targets
            self.z[i] = OH.z_offset_from_coefficients(*cde, t)
            m = len(cde[0])
            for signs in (np.ones((3, m)), -np.ones((3, m)), rng.choice([-1.0, 1.0], (3, m)), rng.choice([-1.0, 1.0], (3, m))):
                z1 = OH.z_offset_from_coefficients(*(np.nextafter(v, (s * np.inf).astype(np.float32)) for v, s in zip(cde, signs)), t)
                d = abs(z1 - self.z[i])
                self.moved[i] = max(self.moved[i], d if np.isfinite(d) else np.inf)
        self.z32 = self.z.astype(np.float32)
        # the issue's bound max(1e-3 mm, k ulp32(|z|)): k = 1 (the final cast of a value that may sit on a rounding boundary)
        # + 4 x the oracle's own movement in ulp32 (the factor 4: summation order)
        with np.errstate(invalid='ignore'):
            self.k = 1.0 + 4.0 * self.moved / ulp32(self.z)
            self.tol = np.maximum(1e-3, self.k * ulp32(self.z))
            # held: the oracle itself is stable within 1 mm, or within the float32 spacing of its own answer (the collapsed
            # family's offsets are ~1e7 mm, spacing 1 to 2 mm)
            self.held = np.isfinite(self.z) & (self.moved <= np.maximum(1.0, ulp32(self.z)))

    def check_z(self, z_dev, what=''):
        """Asserts the device z offsets [n]; returns (worst |dz| mm, worst |dz| / tolerance) over the held problems."""
        z_dev = np.asarray(z_dev, np.float64)
        finite = np.isfinite(self.z)
        assert np.isfinite(z_dev[finite]).all(), f'{what}: NaN where scipy is finite at {np.flatnonzero(finite & ~np.isfinite(z_dev))}'
        assert (~self.held).mean() <= 0.02, f'{what}: {(~self.held).sum()} of {self.n} problems excluded (cap 2 %)'
        err = np.abs(z_dev - self.z32.astype(np.float64))[self.held]
        ratio = err / self.tol[self.held]
        print(f'{what}: z offset worst |d| {err.max():.3e} mm, worst |d| / tol {ratio.max():.3f}, largest k {self.k[self.held].max():.1f}, '
              f'excluded {(~self.held).sum()}')
        assert (ratio <= 1.0).all(), (what, np.flatnonzero(self.held)[ratio > 1.0], err.max(), ratio.max())
        return float(err.max()), float(ratio.max())

    def check_poses(self, got, ref, what=''):
        """Poses [n, J, 3] placed with the device's z against the oracle's placed with scipy's.  A point is ray * (delta_z + z):
        |ray| <= sqrt(1 + x^2 + y^2) < 1.2 here (z component 1, |x|, |y| < 0.4), a rotation keeps the length, so a z offset that
        is off by dz moves no coordinate by more than 1.2 dz (2 dz allowed), plus the fp32 roundings of the chain that the
        placement tests already hold to 1e-6 of the pose's largest coordinate."""
        got, ref = np.asarray(got, np.float64)[self.held], np.asarray(ref, np.float64)[self.held]
        assert np.abs(self.cam).max() < 1.2
        err = np.abs(got - ref).max(axis=(1, 2))
        bound = 2.0 * self.tol[self.held] + 1e-6 * np.abs(ref).max(axis=(1, 2))
        assert (err <= bound).all(), (what, np.flatnonzero(self.held)[err > bound], (err / bound).max())
        return float((err / bound).max())


_BONE_CASES = {}


def bone_case(dataset, family, per_pose):
    """The corpus case, computed once per process (its reference is ~650 scipy solves)."""
    key = (dataset, family, bool(per_pose))
    if key not in _BONE_CASES:
        _BONE_CASES[key] = BoneCase(*key)
    return _BONE_CASES[key]
