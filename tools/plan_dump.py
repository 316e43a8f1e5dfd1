"""Everything the C ABI shows of a plan, as one sha256 per spec (or, with --full, as tables that can be diffed).

    python tools/plan_dump.py [--lib PATH] [--full] [--only KEY] [--out FILE.json]

For each spec of a fixed matrix a plan is created with max_batch 256 and the following is hashed, in order: the raw bytes of
every MetroParamInfo, the raw bytes of every MetroLayerInfo, workspace_bytes, param_bytes, flops_per_image,
metro_plan_status_offset, and the metro_plan_layer_kernel string of every layer at each batch of BATCHES.  Planning and the
dispatch dry run are host-only: no GPU is needed.  A spec metro_plan_create rejects is recorded as 'rejected: <error text>'.

tests/test_plan_snapshot.py holds the in-tree library to tests/golden/plan_tables_v1.json, which this tool wrote from a
library built from the sources of the commit BEFORE a change to the planner (--lib that library, --out the golden file).
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from metro_pose3d_amd import _lib  # noqa: E402
from metro_pose3d_amd.spec import ModelSpec  # noqa: E402

MAX_BATCH = 256
BATCHES = (1, 8, 16, 32, 64, 128, 256)
PRECISIONS = {'f16': _lib.METRO_PREC_F16, 'f32': _lib.METRO_PREC_F32, 'f32m': _lib.METRO_PREC_F32M, 'f64': _lib.METRO_PREC_F64}
_USED = ('metro_plan_create', 'metro_plan_destroy', 'metro_plan_workspace_bytes', 'metro_plan_param_bytes', 'metro_plan_num_params',
         'metro_plan_param_info', 'metro_plan_num_layers', 'metro_plan_layer_info', 'metro_plan_flops_per_image',
         'metro_plan_layer_kernel', 'metro_plan_status_offset', 'metro_last_error')


def matrix():
    """[(key, ModelSpec, precision name)]: the core matrix, then the secondary axes for f16 and f64."""
    out = []

    def add(prec, **kw):
        spec = ModelSpec(**kw)
        key = (f'r{spec.arch}-s{spec.stride}-{"c" if spec.centered_stride else "u"}-{spec.dataset}-w{spec.base_width}'
               f'-p{spec.proc_side}-{prec}')
        if key not in [k for k, _, _ in out]:
            out.append((key, spec, prec))

    for arch in (50, 101):
        for stride in (4, 8, 16, 32):
            for centered in (True, False):
                for prec in ('f16', 'f32', 'f32m', 'f64'):
                    add(prec, arch=arch, stride=stride, centered_stride=centered)
    for arch in (50, 101):
        for stride in (4, 8, 16, 32):
            for centered in (True, False):
                for prec in ('f16', 'f64'):
                    base = dict(arch=arch, stride=stride, centered_stride=centered)
                    for dataset in ('many19', 'merged'):
                        add(prec, dataset=dataset, **base)
                    for width in (8, 32):
                        add(prec, base_width=width, **base)
                    add(prec, proc_side=384, **base)
                    if stride == 32:
                        add(prec, proc_side=64, **base)
    return out


def open_lib(path=None):
    """The in-tree library, or the one at `path` (a library of another commit: only the entries this tool calls are bound)."""
    if path is None:
        return _lib.load()
    import torch  # noqa: F401  (first, as _lib.load does: it brings the HIP runtime the library must share)
    lib = C.CDLL(os.path.abspath(path))
    for name in _USED:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def tables(lib, spec: ModelSpec, prec: str):
    """(params, layers, scalars, kernels) of the plan, or the rejection text."""
    cs = spec.to_c(PRECISIONS[prec])
    plan = C.c_void_p()
    if lib.metro_plan_create(C.byref(cs), MAX_BATCH, C.byref(plan)) != 0:
        return 'rejected: ' + lib.metro_last_error().decode(errors='replace')
    try:
        params, layers, kernels = [], [], []
        for i in range(lib.metro_plan_num_params(plan)):
            pi = _lib.MetroParamInfo()
            assert lib.metro_plan_param_info(plan, i, C.byref(pi)) == 0
            params.append(pi)
        buf = C.create_string_buffer(1024)
        for i in range(lib.metro_plan_num_layers(plan)):
            li = _lib.MetroLayerInfo()
            assert lib.metro_plan_layer_info(plan, i, C.byref(li)) == 0
            layers.append(li)
            row = []
            for n in BATCHES:
                st = lib.metro_plan_layer_kernel(plan, i, n, buf, len(buf))
                row.append(buf.value.decode() if st == 0 else f'status {st}: ' + lib.metro_last_error().decode(errors='replace'))
            kernels.append(row)
        scalars = (lib.metro_plan_workspace_bytes(plan), lib.metro_plan_param_bytes(plan),
                   lib.metro_plan_flops_per_image(plan), lib.metro_plan_status_offset(plan))
        return params, layers, scalars, kernels
    finally:
        lib.metro_plan_destroy(plan)


def digest(t) -> str:
    if isinstance(t, str):
        return t
    params, layers, scalars, kernels = t
    h = hashlib.sha256()
    for s in params + layers:
        h.update(bytes(s))
    h.update(struct.pack('<qqdq', *scalars))
    for row in kernels:
        for k in row:
            h.update(k.encode() + b'\0')
    return h.hexdigest()


def _fields(s):
    return ' '.join(f'{name}={getattr(s, name).decode() if isinstance(getattr(s, name), bytes) else getattr(s, name)}'
                    for name, _ in s._fields_)


def full(key, t) -> str:
    if isinstance(t, str):
        return f'== {key}\n{t}\n'
    params, layers, scalars, kernels = t
    lines = [f'== {key}', 'workspace_bytes=%d param_bytes=%d flops_per_image=%r status_offset=%d' % scalars]
    lines += [f'param {i}: {_fields(p)}  raw={hashlib.sha256(bytes(p)).hexdigest()[:12]}' for i, p in enumerate(params)]
    for i, (layer, row) in enumerate(zip(layers, kernels)):
        lines.append(f'layer {i}: {_fields(layer)}  raw={hashlib.sha256(bytes(layer)).hexdigest()[:12]}')
        lines += [f'layer {i} batch {n}: {k}' for n, k in zip(BATCHES, row)]
    return '\n'.join(lines) + '\n'


def snapshot(lib, only=None) -> dict:
    return {key: digest(tables(lib, spec, prec)) for key, spec, prec in matrix() if only in (None, key)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', help='libmetro_hip.so to read (default: the in-tree library)')
    ap.add_argument('--full', action='store_true', help='print the tables instead of the hashes')
    ap.add_argument('--only', help='one spec key of the matrix')
    ap.add_argument('--out', help='write {spec key: sha256} as JSON here instead of printing it')
    a = ap.parse_args()
    lib = open_lib(a.lib)
    if a.full:
        for key, spec, prec in matrix():
            if a.only in (None, key):
                sys.stdout.write(full(key, tables(lib, spec, prec)))
        return 0
    text = json.dumps(snapshot(lib, a.only), indent=0, sort_keys=True) + '\n'
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
