"""Records profiles/view_fusion_parity.json:
  scene/<name>                   the two-peaked scene of the design note on the fp64 restatement (tests/view_fusion_ref.py): the
                                 error in mm of the uniform and the covariance-weighted triangulation of the means and of the
                                 fused mean, with peak, agreement and edge (needs no device)
  gpu/<head>/persons<P>          the worst deviation of what a bound forward wrote on hand-filled marginals from the restatement
                                 (tests/test_gpu_view_fusion.py): points in mm, a covariance block over its largest entry, peak,
                                 agreement
Nothing gates on this file: the tests hold the bounds of the issue (view_fusion_ref.POINT_MM, BLOCK_BOUND, STAT_ULPS / STAT_ABS
and the scene's factors), which are written next to the figures.

    python tools/view_fusion_parity.py [--out FILE]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import torch
    from tests import test_view_fusion as TV, view_fusion_ref as VF
    scenes = {'two-peaked': {}, 'wrong-peak-weight-0.7': dict(wrong_weight=0.7), 'four-cameras': dict(angles_deg=(0.0, 90.0, 180.0, 270.0)),
              'clean': dict(wrong_weight=0.0), 'two-cameras': dict(angles_deg=(0.0, 120.0))}
    rec = {'scene': {name: TV._errors(**kw) for name, kw in scenes.items()},
           'bounds': {'points_mm': VF.POINT_MM, 'block': VF.BLOCK_BOUND, 'stat_ulps': VF.STAT_ULPS, 'stat_abs': VF.STAT_ABS,
                      'scene': 'fused <= weighted / 3 and <= one grid step (80 mm); clean scene: fused <= 10 mm'},
           'what': 'scene: errors in mm against the true joint, G = 16 over 1200 mm, floor 1e-6, the cube centred on the '
                   'covariance-weighted triangulation; gpu: worst deviation from the fp64 restatement per key; the tests assert '
                   '`bounds`, not these figures'}
    if torch.cuda.is_available():
        from tests import test_gpu_view_fusion as TG
        rec['worst'] = TG.gpu_deviations(torch.device('cuda', 0))
        rec['device'] = torch.cuda.get_device_name(0)
    else:
        print('view_fusion_parity: no HIP device visible, the scene figures only', file=sys.stderr)
    out = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'view_fusion_parity.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    for name, e in rec['scene'].items():
        print(f'{name:24s} uniform {e["uniform"]:7.1f}  weighted {e["weighted"]:7.1f}  fused {e["fused"]:7.2f} mm  agreement {e["agreement"]:.3f}')
    for key in sorted(rec.get('worst', {})):
        print(f'{key:32s} {rec["worst"][key]}')


if __name__ == '__main__':
    main(sys.argv[1:])
