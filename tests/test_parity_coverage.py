"""The parity modes (precision 'f64', 'f32', 'f32m') held like the f16 path: a dispatch closure on the CPU, one launch per
(kernel id, layer shape) pair through the C ABI against fp64, whole forwards across the tile threshold and off crop side 256.

What the parity modes dispatch (a dry run: Engine(spec, None, prec).layer_kernels(n) needs no device): conv_igemm_f64acc for
'f64' (fp64 storage; the stem reads the fp32 image: in32,act64) and 'f32' (in32,act32), conv_igemm_f32 for 'f32m', the fp32 /
fp64 max-pool, and the fp64-accumulating soft-argmax on fp32 or fp64 logits.  conv_igemm_f64acc picks 64- or 128-cout tiles
from the BATCH (`small = c_out <= 64 || tiles128 < 512`), so which instantiation a layer runs on changes with the call size:
the 128-cout tiles carry every layer of an f64 forward from about 16 crops on.

  * test_parity_id_closure (CPU): every id the three modes dispatch over the whole supported grid (crop sides 64 .. 512, both
    archs, four strides, three heads, every call size 1 .. 256) is launched by a case below.
  * test_parity_pair_closure (CPU): every (id, SHAPE_KEY) pair at crop side 256 over every arch / stride / head / call size,
    and of RN50 at sides 224, 288 and 416 (odd maps down to 7 x 7, the 18 x 18 head of 424 channels, 52-wide maps), is launched
    by a case, at the smallest call that reaches it.  The case list is generated from the dry run: a new instantiation cannot
    enter a parity plan without a case.
  * test_parity_launch (`-m gpu`): one case per pair.  A conv case runs two operand sets.  EXACT: dyadic operands
    (helpers.dyadic_conv_operands; prologue scales from {-1.5 .. 1.5}, zero and negative ones included) on which every partial
    sum is exact in fp32 -- checked per case from the reference's condition sums, not assumed -- so the output must EQUAL the
    fp64 tap sum: a dropped, doubled or misplaced tap fails at any K.  GAUSSIAN: the operands of the f16 cases with a random
    sign on the prologue scales, element by element inside the conv contract's bound (test_gpu_conv_contract._check) with the
    kernel's unit roundoff, 2^-53 for conv_igemm_f64acc and 2^-24 for conv_igemm_f32: this is what tells fp64 accumulation from
    fp32.  Every case: the entry point must launch the id the plan names, the output lies NaN-filled between two guard bands,
    the call is laid out from p base images (p = 2 where the map has >= 4096 pixels and c_in c_out >= 2^17, else 4) and every
    position must carry its twin's bits; the reference is computed for the base images only.  The max-pool is held bit for bit
    to max_pool2d over the zero-padded fp64 input, the soft-argmax to the oracle's logits_to_output on planted-peak logits
    (2e-3 mm on fp32 logits, TOL_PARITY_MM on fp64 ones).
  * test_side224_forward_all_modes, test_forward_across_the_tile_threshold (`-m gpu`): whole forwards.

Counts (printed by the closure tests): 25 kernel ids over the grid (22 conv / pool ids, the two partials kernels and their
finalize); 1440 (id, shape) pairs -- 361 first reached at side 256, 355 / 361 / 363 more at sides 224 / 288 / 416; 1440 launch
cases + 5 whole-forward cases = 1445 new GPU cases.
Measured on the MI355X: the file's GPU cases take 225 s in all (sides 256 + 224 and the forwards 78 s, sides 288 + 416 147 s);
the slowest case is f32:rn50-s4-h36m-side416-b4:block3/unit_1/conv2 on conv_igemm_f64acc<in32,act32,128x128,v2> at 3.2 s (4
crops of a 104 x 104 map, 256 -> 256 3x3, each with its own fp64 reference), the mean case 0.16 s.  Worst Gaussian-set
|err| / bound: conv_igemm_f64acc with fp64 store 0.007, with fp32 store 0.50 (the half ulp of the one fp32 rounding against
the bound's 2^-23 |y|), conv_igemm_f32 0.012.  The CPU closures take 28 s.
"""
import copy
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, synth
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H
from tests.test_kernel_coverage import (GRID_ARCHS, GRID_BATCHES, GRID_DATASETS, GRID_SIDES, GRID_STRIDES, PAIR_SPECS, SHAPE_KEY,
                                        DryRun, _same_backbone, spec_name)

PARITY = ('f64', 'f32', 'f32m')
PAIR_SIDES_RN50 = (224, 288, 416)       # beyond PAIR_SPECS (side 256): odd maps, the 18-wide head, 52-wide maps
F32, F64 = _lib.METRO_F32, _lib.METRO_F64
CONV_FAMILIES = ('conv_igemm_f64acc<', 'conv_igemm_f32<')


def pair_specs():
    return PAIR_SPECS + [ModelSpec(50, s, d, proc_side=side) for side in PAIR_SIDES_RN50 for s in GRID_STRIDES for d in GRID_DATASETS]


_UNIVERSE = {}


def parity_universe():
    """{(kernel id, shape key): (precision, spec, n, layer index, layer name)} over PARITY x pair_specs() x GRID_BATCHES: the first
    mode and spec at the smallest n that reaches each pair.  One dry run per process."""
    if not _UNIVERSE:
        for prec in PARITY:
            for spec in pair_specs():
                run = DryRun(spec, precision=prec)
                for n in GRID_BATCHES:
                    for i, kid in enumerate(run.kernels(n)):
                        at = _UNIVERSE.get((kid, run.keys[i]))
                        if at is None or n < at[2]:
                            _UNIVERSE[(kid, run.keys[i])] = (prec, spec, n, i, run.names[i])
    return _UNIVERSE


def _cases():
    """One case per pair of the universe, in shape order (the cases of one layer shape share their references)."""
    out = []
    for (kid, key), (prec, spec, n, i, name) in sorted(parity_universe().items(), key=lambda kv: (kv[0][1], kv[0][0])):
        out.append(pytest.param(prec, spec, n, i, kid, id=f'{prec}:{spec_name(spec)}-b{n}:{name}:{kid}'))
    return out


try:
    _CASES = _cases()
except Exception as e:  # noqa: BLE001  (library not built: the CPU tests below report it)
    _CASES = [pytest.param(None, None, 0, -1, str(e), id='library-missing')]


def launched(cases):
    """{(kernel id, shape key)} of what the launch cases run, read back from a dry run of each case's own (mode, spec, n, layer)."""
    out, runs = set(), {}
    for p in cases:
        prec, spec, n, i, kid = p.values
        run = runs.get((prec, spec))
        if run is None:
            run = runs[(prec, spec)] = DryRun(spec, precision=prec)
        assert run.kernels(n, [i]) == [kid], p.id
        out.add((kid, run.keys[i]))
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def missing_ids(cases):
    """Ids the three modes dispatch over the whole grid that no case launches: {id: the first plan that reaches it}."""
    have = {part for kid, _ in launched(cases) for part in kid.split(' & ')}
    missing, n_ids = {}, set()
    for prec in PARITY:
        for side in GRID_SIDES:
            for arch in GRID_ARCHS:
                for stride in GRID_STRIDES:
                    base = None
                    for ds in GRID_DATASETS:
                        run = DryRun(ModelSpec(arch, stride, ds, proc_side=side), precision=prec)
                        layers = None
                        if base is None:
                            base = run
                        else:
                            assert _same_backbone(base, run), f'{prec}: rn{arch}-s{stride}-{ds} at proc_side {side}: backbone differs'
                            layers = range(run.names.index('logits'), len(run.names))
                        for n in GRID_BATCHES:
                            for kid in run.kernels(n, layers):
                                for part in kid.split(' & '):
                                    n_ids.add(part)
                                    if part not in have:
                                        missing.setdefault(part, f'{prec}: rn{arch}-s{stride}-{ds} at proc_side {side}, batch {n}')
    return missing, n_ids


def test_parity_id_closure():
    """Every kernel id that precision 'f64', 'f32' or 'f32m' dispatches anywhere on the supported grid (test_dispatch_closure's:
    408 specs x 256 call sizes, one plan per spec and mode, the other heads asked for their head layers after the assertion
    that their backbone equals h36m's) is launched by a case of test_parity_launch."""
    assert _CASES[0].values[0] is not None, f'libmetro_hip.so could not be loaded: {_CASES[0].values[4]}'
    missing, ids = missing_ids(_CASES)
    print(f'\n{len(ids)} kernel ids dispatched by the parity modes over the grid')
    assert not missing, 'dispatched by a parity mode but launched by no GPU case:\n' + '\n'.join(f'  {k}: {w}' for k, w in sorted(missing.items()))
    assert len(ids) >= 24, sorted(ids)


def test_parity_pair_closure():
    """Every (kernel id, layer shape) pair of the parity modes at crop side 256 (every arch / stride / head / call size) and of
    RN50 at sides 224, 288 and 416 is launched by a case, at the smallest call that reaches it."""
    assert _CASES[0].values[0] is not None, f'libmetro_hip.so could not be loaded: {_CASES[0].values[4]}'
    universe = parity_universe()
    have = launched(_CASES)
    sides = {}
    for _, spec, _, _, _ in universe.values():
        sides[spec.proc_side] = sides.get(spec.proc_side, 0) + 1
    print(f'\n{len(universe)} (kernel id, layer shape) pairs (first reached at side: {sorted(sides.items())}); {len(_CASES)} launch cases')
    missing = {pair: at for pair, at in universe.items() if pair not in have}
    assert not missing, 'dispatched by a parity mode but launched by no GPU case:\n' + \
        '\n'.join(f'  {kid}: {prec} {spec_name(spec)}, batch {n}, {name} {dict(zip(SHAPE_KEY, key))}'
                  for (kid, key), (prec, spec, n, i, name) in sorted(missing.items(), key=lambda kv: kv[0]))
    runs = {}
    for p in _CASES:                    # ... at the smallest n that reaches the pair
        prec, spec, n, i, kid = p.values
        if (prec, spec) not in runs:
            runs[(prec, spec)] = DryRun(spec, precision=prec)
        assert n == 1 or runs[(prec, spec)].kernels(n - 1, [i]) != [kid], p.id


def test_the_planner_puts_the_operand_types_where_it_says():
    """f64: the stem reads the fp32 image and stores fp64 (in32,act64), every other conv is in64,act64; f32: in32,act32
    throughout; f32m: conv_igemm_f32.  The pool and the soft-argmax follow the storage type."""
    for spec in (ModelSpec(50, 16, 'h36m'), ModelSpec(101, 8, 'merged', proc_side=224)):
        for n in (1, 64):
            for prec, stem, rest, pool, sa in (('f64', 'in32,act64', 'in64,act64', 'f64', 'logits64'), ('f32', 'in32,act32', 'in32,act32', 'f32', 'logits32'),
                                               ('f32m', None, None, 'f32', 'logits32')):
                eng = Engine(spec, None, prec, max_batch=n)
                names = [li.name.decode() for li in eng.layer_infos()]
                ids = eng.layer_kernels(n)
                assert names[:2] == ['conv1', 'pool1'] and names[-2:] == ['logits', 'softargmax']
                assert ids[1] == f'maxpool3x3s2_zeropad<{pool}>'
                assert ids[-1] == f'softargmax_partial<acc64,{sa}> & softargmax_finalize<acc64>'
                convs = ids[2:-1]
                if prec == 'f32m':
                    assert ids[0] == 'conv_igemm_f32<64x128,bk32>' and all(k.startswith('conv_igemm_f32<') and ',v4' in k for k in convs)
                else:
                    assert ids[0] == f'conv_igemm_f64acc<{stem},128x64>', ids[0]
                    assert all(k.startswith(f'conv_igemm_f64acc<{rest},128x') and ',v2' in k for k in convs), convs


def tile_threshold_layers(spec, prec, n):
    """The layers of a plan that run 128-cout tiles at n crops and 64-cout tiles at n // 2."""
    run = DryRun(spec, precision=prec)
    return [i for i, (a, b) in enumerate(zip(run.kernels(n), run.kernels(n // 2))) if ',128x128' in a and ',128x64' in b]


def test_the_tile_follows_the_batch():
    """conv_igemm_f64acc's tile is chosen from the call size: the same layer shape has a 128x128 id and a 128x64 id."""
    for prec in ('f64', 'f32'):
        by_shape = {}
        for (kid, key), _ in parity_universe().items():
            if kid.startswith('conv_igemm_f64acc<' + ('in64' if prec == 'f64' else 'in32,act32')):
                by_shape.setdefault(key, set()).add('128x128' in kid)
        assert any(v == {True, False} for v in by_shape.values()), prec
        assert tile_threshold_layers(THRESHOLD_SPEC, prec, THRESHOLD_N), prec
        assert not tile_threshold_layers(THRESHOLD_SPEC, prec, THRESHOLD_N - 2), prec       # the smallest such even call


# ---- GPU: one launch per pair ---------------------------------------------------------------------------------------------
_REFS = {}          # the references of the layer shape the cases are at (cleared when the shape changes: _CASES is in shape order)
RATIOS = {}         # kernel family -> worst Gaussian-set |err| / bound so far (printed per case)


def _shared(key, what, make):
    if _REFS.get('shape') != key:
        _REFS.clear()
        _REFS['shape'] = key
    if what not in _REFS:
        _REFS[what] = make()
    return _REFS[what]


def _noted(lib):
    return lib.metro_last_kernel_id().decode()


def base_images(li):
    """p of the issue: 2 base images where the map has >= 4096 pixels and c_in c_out >= 2^17, 4 otherwise."""
    return 2 if li.h_out * li.w_out >= 4096 and li.c_in * li.c_out >= 2 ** 17 else 4


def _desc(li, n, in_dtype):
    rs, ro = li.res_stride, li.res_offset
    res_h = li.h_out if rs == 1 else 2 * li.h_out
    assert not li.has_residual or (li.h_out - 1) * rs + ro < res_h
    return H.conv_desc(n, li.h_in, li.c_in, li.h_out, li.c_out, 0, li.stride, li.dilation, prologue=bool(li.has_prologue), relu=bool(li.relu),
                       residual=bool(li.has_residual), res_h=res_h, res_stride=rs, res_offset=ro, out_dtype=li.out_dtype, in_dtype=in_dtype,
                       w_in=li.w_in, w_out=li.w_out, kh=li.kh, kw=li.kw, pad_top=li.pad_top, pad_left=li.pad_left)


def _exact_set(key, d):
    """(x, w, b, pro, res, y): dyadic operands of the base images and their exact result; the value range is narrowed until
    every partial sum is exact in fp32 (no layer of the grid needs it: K = 4608 gives a <= 4608 * 2.5 at most)."""
    for lim in (8, 4, 2, 1):
        rng = np.random.default_rng([zlib.crc32(repr(key).encode()), lim])
        x, w, b, pro, res = H.dyadic_conv_operands(rng, d, lim)
        y, a = H.ref_conv_desc(d, x, w, b, pro=pro, pro_round=None, res=res)
        if H.exact_sum_condition(a, d.has_prologue):
            return x, w, b, pro, res, y
    raise AssertionError(f'no dyadic value range keeps the partial sums of {dict(zip(SHAPE_KEY, key))} exact in fp32')


def _gaussian_values(key, d):
    """The operands of test_kernel_coverage._conv in fp64, with a random sign on the prologue scales."""
    rng = np.random.default_rng([zlib.crc32(repr(key).encode()), 77])
    k = d.kh * d.kw * d.c_in
    x = rng.standard_normal((d.n, d.h_in, d.w_in, d.c_in))
    if not d.has_prologue and d.kh == 3:
        x = np.maximum(x, 0)
    w = rng.standard_normal((d.c_out, d.kh, d.kw, d.c_in)) * np.sqrt(2.0 / k)
    b = rng.standard_normal(d.c_out) * 0.1
    pro = (rng.uniform(0.5, 1.5, d.c_in) * rng.choice([-1.0, 1.0], d.c_in), rng.standard_normal(d.c_in) * 0.2) if d.has_prologue else None
    res = rng.standard_normal((d.n, d.res_h, d.res_w, d.c_out)) if d.has_residual else None
    return x, w, b, pro, res


def _gaussian_set(key, d, np_in, np_w, np_act):
    """... rounded to the types the kernel reads them in, and (y, a) of helpers.ref_conv_desc on exactly those values."""
    types = (d.n, np_in, np_w, np_act)
    if _REFS.get('shape') == key and types in _REFS:
        return _REFS[types]
    x, w, b, pro, res = _shared(key, ('gauss', d.n), lambda: _gaussian_values(key, d))
    x, w, b = x.astype(np_in), w.astype(np_w), b.astype(np_w)
    pro = None if pro is None else (pro[0].astype(np_w), pro[1].astype(np_w))
    res = None if res is None else res.astype(np_act)
    y, a = H.ref_conv_desc(d, x, w, b, pro=pro, pro_round=np.float32 if np_w is np.float32 else None, res=res)
    _REFS[types] = (x, w, b, pro, res, y, a)
    return _REFS[types]


def _conv(lib, cuda, li, n, kid, what, assign=None):
    from tests.test_gpu_conv_contract import _check, _guarded, _guards_intact
    f32m = kid.startswith('conv_igemm_f32<')
    np_in = np.float64 if 'in64' in kid else np.float32
    np_act = np.float64 if li.out_dtype == F64 else np.float32
    np_w = np.float32 if f32m else np.float64
    assert f32m or f'act{np_act().itemsize * 8}' in kid, kid
    key = tuple(getattr(li, f) for f in SHAPE_KEY if f != 'out_dtype')          # (the modes share a layer shape's values)
    p = min(base_images(li), n)
    if assign is None:
        assign = H.crop_assignment(n, p, zlib.crc32(what.encode()))
    assert len(assign) == n and int(np.max(assign)) + 1 == p
    d = _desc(li, n, F64 if np_in is np.float64 else F32)
    dp = copy.copy(d)
    dp.n = p
    fn = lib.metro_conv_f32m if f32m else lib.metro_conv_f64acc
    t_act = torch.float64 if np_act is np.float64 else torch.float32
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(cuda)

    def run(x, w, b, pro, res):
        tx = H.lay_out_twins(dev(x, np_in), assign)
        tr = None if res is None else H.lay_out_twins(dev(res, np_act), assign)
        tw, tb = dev(w, np_w), dev(b, np_w)
        ts, tsh = (dev(pro[0], np_w), dev(pro[1], np_w)) if pro is not None else (None, None)
        out, buf = _guarded((n, d.h_out, d.w_out, d.c_out), t_act, cuda)
        check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
        try:
            check(fn(C.byref(d), H.ptr(tx), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr), H.ptr(out), None), what)
            torch.cuda.synchronize()
            noted = _noted(lib)
        finally:
            lib.metro_kernel_notes(0)
        assert noted == kid, f'the entry point launched {noted}, the plan names {kid}'
        assert _guards_intact(buf), f'{what}: a store landed outside the output tensor'
        H.assert_twins(out, assign, p, what)
        return out[:p].cpu().numpy()

    # ---- exact set: the same dyadic values in every mode, the result must equal the fp64 tap sum
    x, w, b, pro, res, y = _shared(key, ('exact', p), lambda: _exact_set(key, dp))
    got = run(x, w, b, pro, res)
    assert np.isfinite(got).all(), f'{what}: elements not written (or not finite) on the exact set'
    bad = got.astype(np.float64) != y
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements differ from the exact result on dyadic operands; first at '
                           f'{tuple(np.argwhere(bad)[0])}: got {got[tuple(np.argwhere(bad)[0])]!r} want {y[tuple(np.argwhere(bad)[0])]!r}')
    # ---- Gaussian set: element by element inside the contract's bound with the kernel's unit roundoff
    x, w, b, pro, res, y, a = _gaussian_set(key, dp, np_in, np_w, np_act)
    got = run(x, w, b, pro, res)
    u = 2.0 ** -24 if f32m else 2.0 ** -53
    ratio = _check(got, y, a, dp, u, 2.0 ** -52 if np_act is np.float64 else 2.0 ** -23, what=what)
    fam = kid.split('<')[0] + ('' if f32m else '<act64>' if np_act is np.float64 else '<act32>')
    RATIOS[fam] = max(RATIOS.get(fam, 0.0), ratio)
    print(f'\n[parity] {what}: Gaussian set worst |err| / bound {ratio:.3f} (family {fam}: {RATIOS[fam]:.3f} so far)')


def _pool(lib, cuda, li, n, kid, what, assign=None):
    from tests.test_gpu_conv_contract import _guarded, _guards_intact
    p = min(4, n)
    if assign is None:
        assign = H.crop_assignment(n, p, zlib.crc32(what.encode()))
    assert len(assign) == n and int(np.max(assign)) + 1 == p
    tdt = torch.float64 if li.out_dtype == F64 else torch.float32
    gen = torch.Generator(device=cuda)
    gen.manual_seed(zlib.crc32(what.encode()))
    base = torch.randn((p, li.h_in, li.w_in, li.c_in), generator=gen, device=cuda, dtype=tdt)
    base[p - 1, :, :, ::2] = -base[p - 1, :, :, ::2].abs() - 0.5      # all-negative channels: their border windows must see the zero pad
    x = H.lay_out_twins(base, assign)
    out, buf = _guarded((n, li.h_out, li.w_out, li.c_in), tdt, cuda)
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        check(lib.metro_maxpool3x3s2_zeropad(H.ptr(x), H.ptr(out), n, li.h_in, li.w_in, li.c_in, li.out_dtype, None), what)
        torch.cuda.synchronize()
        noted = _noted(lib)
    finally:
        lib.metro_kernel_notes(0)
    assert noted == kid, f'the entry point launched {noted}, the plan names {kid}'
    assert _guards_intact(buf), f'{what}: a store landed outside the output tensor'
    H.assert_twins(out, assign, p, what)
    xp = torch.nn.functional.pad(base.cpu().double().permute(0, 3, 1, 2), (1, 1, 1, 1))
    want = torch.nn.functional.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1)
    assert want.shape[1:3] == (li.h_out, li.w_out)
    assert torch.equal(out[:p].cpu().double(), want), what
    assert (want[p - 1, 0, :, ::2] == 0).all() and (want[p - 1, 1:, 1:, ::2] < 0).all()


def _softargmax(lib, cuda, spec, n, kid, what, assign=None):
    """N(0, 4) logits plus one planted peak per (image, joint) at a random voxel (test_kernel_coverage._softargmax), in the
    type the mode stores its logits in."""
    from oracle.forward import logits_to_output
    from tests.test_gpu_forward import TOL_PARITY_MM
    logits64 = 'logits64' in kid
    side, j, dd = spec.heatmap_side, spec.skeleton.n_head, spec.depth
    p = min(4, n)
    if assign is None:
        assign = H.crop_assignment(n, p, zlib.crc32(what.encode()))
    assert len(assign) == n and int(np.max(assign)) + 1 == p
    gen = torch.Generator(device=cuda)
    gen.manual_seed(zlib.crc32(what.encode()))
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    base = torch.randn((p, side, side, dd * j), generator=gen, device=cuda, dtype=torch.float64 if logits64 else torch.float32) * 4.0
    for i in range(p):
        for jj in range(j):
            h, w, dz = (int(v) for v in rng.integers(0, (side, side, dd)))
            base[i, h, w, dz * j + jj] += 12.0
    logits = H.lay_out_twins(base, assign)
    precise = 2 if logits64 else 1
    cs = spec.to_c(_lib.METRO_PREC_F64 if logits64 else _lib.METRO_PREC_F32)
    scratch = torch.empty(lib.metro_softargmax_scratch_bytes(n, side, j), dtype=torch.uint8, device=cuda)
    poses = torch.full((n, spec.skeleton.n_out, 3), float('nan'), dtype=torch.float32, device=cuda)
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        check(lib.metro_softargmax(H.ptr(logits), n, C.byref(cs), precise, H.ptr(scratch), H.ptr(poses), None), what)
        torch.cuda.synchronize()
        noted = _noted(lib)
    finally:
        lib.metro_kernel_notes(0)
    assert noted == kid, f'the entry point launched {noted}, the plan names {kid}'
    H.assert_twins(poses, assign, p, what)
    want = logits_to_output(H.oracle_spec(spec), base.cpu().double().numpy()).numpy()
    got = poses[:p].cpu().numpy()
    assert np.isfinite(got).all(), what
    dmm = np.abs(got - want).max()
    bar = TOL_PARITY_MM if logits64 else 2e-3
    print(f'\n[parity] {what}: poses {dmm:.2e} mm (bar {bar:g})')
    assert dmm <= bar, f'{what}: poses {dmm} mm from the exact soft-argmax of the same logits'
    assert side < 4 or np.abs(want).max() > 50.0, np.abs(want).max()       # the planted peaks pull the joints off the centre


@pytest.mark.gpu
@pytest.mark.parametrize('prec,spec,n,layer,kid', _CASES)
def test_parity_launch(lib, cuda, prec, spec, n, layer, kid):
    assert prec is not None, f'libmetro_hip.so could not be loaded at collection time: {kid}'
    parity_launch(lib, cuda, prec, spec, n, layer, kid)


def parity_launch(lib, cuda, prec, spec, n, layer, kid, assign=None):
    """One launch of `layer` of the `prec` plan of `spec` at call size n, held as the module docstring says.  `assign`: the twin
    layout (default: crop_assignment seeded by the case)."""
    eng = Engine(spec, None, prec, max_batch=n)
    li = eng.layer_infos()[layer]
    assert eng.layer_kernels(n)[layer] == kid
    what = f'{prec} {spec_name(spec)} b{n} {li.name.decode()} {kid}'
    if li.kind == _lib.LAYER_SOFTARGMAX:
        _softargmax(lib, cuda, spec, n, kid, what, assign)
    elif li.kind == _lib.LAYER_POOL:
        _pool(lib, cuda, li, n, kid, what, assign)
    else:
        assert li.kind == _lib.LAYER_CONV and kid.startswith(CONV_FAMILIES), (li.kind, kid)
        _conv(lib, cuda, li, n, kid, what, assign)


# ---- GPU: whole forwards ----------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(spec, n, dtype):
    """(params, images, poses of the oracle in `dtype`) of a spec's seeded synthetic model: computed once per process."""
    from oracle import forward as OF
    k = (spec_name(spec), n)
    if k not in _ORACLE:
        params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(spec.arch, spec.stride))
        _ORACLE[k] = {'params': params, 'images': synth.make_images(n, spec.proc_side)}
    e = _ORACLE[k]
    if dtype not in e:
        e[dtype] = OF.forward(H.oracle_spec(spec), e['params'], e['images'], dtype).numpy().astype(np.float64)
    return e['params'], e['images'], e[dtype]


SIDE224_SPEC = ModelSpec(50, 8, 'many19', proc_side=224)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', PARITY)
def test_side224_forward_all_modes(cuda, prec):
    """RN50-s8 `many19` at crop side 224 (56 / 28-wide maps, rate-2 and rate-4 3x3 layers at 256 and 512 channels, a 28 x 28
    head of 152 channels), 3 crops, against the fp64 oracle with the bars of test_full_rn50_s16_all_modes."""
    from tests.test_gpu_forward import TOL_F32_STORAGE_MM, TOL_PARITY_MM
    spec = SIDE224_SPEC
    params, images, ref = _oracle(spec, 3, torch.float64)
    got = Engine(spec, params, prec, max_batch=3, device=cuda).forward(torch.from_numpy(images).to(cuda)).cpu().numpy()
    assert np.isfinite(got).all()
    e = np.abs(got - ref)
    if prec == 'f32m':      # as close to exact math as the CPU fp32 restatement of the graph is (two samples of the same rounding noise)
        ecpu = np.abs(_oracle(spec, 3, torch.float32)[2] - ref)
        print(f'\n[parity] f32m at side 224: max {e.max():.2e} mean {e.mean():.2e} mm; CPU fp32 restatement: max {ecpu.max():.2e} mean {ecpu.mean():.2e} mm')
        assert e.max() <= max(2.5 * ecpu.max(), 2e-3) and e.mean() <= max(2.0 * ecpu.mean(), 5e-4), (e.max(), ecpu.max(), e.mean(), ecpu.mean())
    else:
        tol = TOL_PARITY_MM if prec == 'f64' else TOL_F32_STORAGE_MM
        print(f'\n[parity] {prec} at side 224: max {e.max():.2e} mm (bar {tol:g})')
        assert e.max() <= tol, (prec, e.max())


THRESHOLD_SPEC = ModelSpec(50, 32, 'h36m')
THRESHOLD_N = 8         # block1's 256-cout layers on 64 x 64 maps: 2 x 32 n tiles of 128 x 128 >= 512 from 8 crops on


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_forward_across_the_tile_threshold(cuda, prec):
    """conv_igemm_f64acc runs 128-cout tiles at THRESHOLD_N crops and 64-cout tiles at half as many on some layers (asserted from
    the dry run).  The tile changes which block computes an element, not the order its products are summed in: the call and its
    two halves give the same bits, at the poses and at the output of the first such layer; the first 2 crops are held to the
    fp64 oracle."""
    from tests.test_gpu_forward import TOL_F32_STORAGE_MM, TOL_PARITY_MM
    spec, n = THRESHOLD_SPEC, THRESHOLD_N
    layers = tile_threshold_layers(spec, prec, n)
    assert layers, 'no layer crosses the tile threshold between n / 2 and n crops'
    params, images, ref = _oracle(spec, 2, torch.float64)
    x = torch.from_numpy(synth.make_images(n, spec.proc_side)).to(cuda)
    assert np.array_equal(x[:2].cpu().numpy(), images)
    eng = Engine(spec, params, prec, max_batch=n, device=cuda)
    whole = eng.forward(x).clone()
    halves = torch.cat([eng.forward(x[:n // 2]).clone(), eng.forward(x[n // 2:]).clone()])
    assert torch.isfinite(whole).all() and torch.equal(whole, halves), f'{prec}: {n} crops and 2 x {n // 2} differ'
    i = layers[0]
    t = eng.forward_upto(x, i)
    th = torch.cat([eng.forward_upto(x[:n // 2], i), eng.forward_upto(x[n // 2:], i)])
    assert torch.isfinite(t).all() and torch.equal(t, th), f'{prec}: layer {i} differs between {n} crops and 2 x {n // 2}'
    e = np.abs(whole[:2].cpu().numpy() - ref).max()
    tol = TOL_PARITY_MM if prec == 'f64' else TOL_F32_STORAGE_MM
    print(f'\n[parity] {prec} across the tile threshold: max {e:.2e} mm (bar {tol:g})')
    assert e <= tol, (prec, e)
