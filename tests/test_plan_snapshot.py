"""The planner's whole output, byte for byte, against a snapshot taken BEFORE the planner was last changed (no GPU needed).

tools/plan_dump.py hashes, for every spec of its matrix (arch x stride x centered_stride x precision, plus datasets, base
widths and crop sides for f16 and f64), everything the C ABI shows of the plan at max_batch 256: every MetroParamInfo and
MetroLayerInfo (raw bytes), the workspace / parameter sizes, the flops, the status offset and the kernel every layer dispatches
to at batches 1 ... 256.  tests/golden/plan_tables_v1.json holds those hashes; a refactor of csrc/planner.cpp must reproduce
every one of them.  What the snapshot cannot see -- input / residual slots and the parameter indices of the fused groups -- is
held by the GPU tests (test_gpu_forward.py, test_f16_layerwise.py, test_kernel_coverage.py).

After an INTENDED change of the plan (a new fusion, another dispatch): look at the difference first,

    python tools/plan_dump.py --full --only <spec key> --lib <libmetro_hip.so built from the commit before> > before.txt
    python tools/plan_dump.py --full --only <spec key> > after.txt

and, when it is the change you meant and nothing else, write the new golden file with
`python tools/plan_dump.py --out tests/golden/plan_tables_v1.json` in the same commit as the planner change.  Never
regenerate it to make an unintended difference go away: a refactor's golden file comes from the library of the commit before.
"""
import json
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import plan_dump  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plan_tables_v1.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_matrix_is_the_golden_files(golden):
    keys = [k for k, _, _ in plan_dump.matrix()]
    assert len(keys) == len(set(keys))
    assert sorted(keys) == sorted(golden)
    # the core matrix: arch x stride x centered_stride x precision at h36m, base width 64, crop side 256
    core = [k for k in keys if '-h36m-w64-p256-' in k]
    assert len(core) == 2 * 4 * 2 * 4


def test_plans_reproduce_the_snapshot(golden):
    lib = plan_dump.open_lib()
    got = plan_dump.snapshot(lib)
    bad = [k for k in golden if got.get(k) != golden[k]]
    assert not bad, (f'{len(bad)} of {len(golden)} plans differ from tests/golden/plan_tables_v1.json, first: {bad[0]} '
                     f'(python tools/plan_dump.py --full --only {bad[0]} shows its tables)')


def test_snapshot_sees_the_plan(golden):
    """The hash moves with the plan: two specs that differ only in centered_stride share no hash, and a dump has its parts."""
    assert golden['r50-s32-c-h36m-w64-p256-f16'] != golden['r50-s32-u-h36m-w64-p256-f16']
    lib = plan_dump.open_lib()
    key, spec, prec = next(m for m in plan_dump.matrix() if m[0] == 'r50-s32-c-h36m-w64-p256-f16')
    params, layers, scalars, kernels = plan_dump.tables(lib, spec, prec)
    assert len(params) > 100 and len(layers) > 30 and scalars[0] > 0 and scalars[1] > 0 and scalars[2] > 0
    assert all(k and not k.startswith('status') for row in kernels for k in row)
    assert any(layer.fused_flags for layer in layers)      # block1's fused launches are in the tables
