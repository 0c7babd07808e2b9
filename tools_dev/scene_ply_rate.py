"""Scene -> point cloud wall clock: the two-step file pipeline against the in-run fusion, on scene_rate.py's synthetic scene.

    two_step   eval_pointcloud --scene_cache (per-map files), then depth_fusion.main on its output folder
    in_run     eval_pointcloud --scene_cache --fuse --no_map_files (maps staged on the GPU, one scene fusion, the PLY)

Both with --view_num 8 --max_d 128 and synthetic weights, on --views images at 940x490; each run processes the scene twice under
two names (the first pass carries the graph captures) and the 'ring' pass is timed: its depth maps (zz_runtime.txt, files on disk
included) plus, for two_step, depth_fusion.main, for in_run the fusion and PLY write (eth3d_maps.TIMES['fuse']).  The two
PLYs' point coordinates are compared byte for byte.

    python tools_dev/scene_ply_rate.py --out profiles/scene_ply_rate.json [--maps_in_flight cu_split]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atvsnet_amd  # noqa: E402,F401
from atvsnet_amd import FLAGS  # noqa: E402
from atvsnet_amd.atvsnet import depth_fusion as DF, eval_pointcloud as E  # noqa: E402
from atvsnet_amd.tools import ply  # noqa: E402
from fusion_rate import measured_head  # noqa: E402
from scene_rate import write_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=24)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--maps_in_flight', choices=('serial', 'cu_split'), default='serial')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix='scene_ply_rate_')
    n = write_scene(root, 'warm', a.views)
    write_scene(root, 'ring', n)
    rows = {'two_step': [], 'in_run': []}
    plys = {}
    for rep in range(a.reps):
        for mode in ('two_step', 'in_run'):
            FLAGS.reset()
            save = os.path.join(root, 'out_%s_%d' % (mode, rep))
            argv = ['--data_root', root, '--savepath', save, '--view_num', '8', '--max_d', '128', '--synthetic_weights',
                    '--scenes', 'warm,ring', '--maps_in_flight', a.maps_in_flight, '--scene_cache']
            if mode == 'in_run':
                argv += ['--fuse', '--no_map_files']
            E.cli(argv)
            ring = os.path.join(save, 'ring')
            with open(os.path.join(ring, 'zz_runtime.txt')) as f:
                maps_s = float(f.read().split()[1])
            if mode == 'two_step':
                t0 = time.time()
                DF.main(['--dense_folder', ring])
                fuse_s = time.time() - t0
            else:
                fuse_s = E.TIMES['fuse']
            row = {'maps': n, 'maps_s': maps_s, 'fuse_s': fuse_s, 'scene_to_ply_s': maps_s + fuse_s,
                   'maps_per_s': n / maps_s, 'writer_busy_ms_per_map': 1e3 * E.TIMES.get('writer_busy', 0.0) / n}
            rows[mode].append(row)
            plys[mode] = ply.read_ply(os.path.join(ring, 'final3d_model.ply'))
            print(mode, rep, json.dumps(row), flush=True)
            if rep + 1 < a.reps:
                shutil.rmtree(save)
    same = plys['two_step'][0].tobytes() == plys['in_run'][0].tobytes()
    summary = {'parent_commit': measured_head(), 'views': n, 'view_num': 8, 'max_d': 128, 'size': '940x490',
               'maps_in_flight': a.maps_in_flight, 'points': int(len(plys['in_run'][0])), 'xyz_bytes_equal': same, 'runs': rows}
    for mode, r in rows.items():
        summary[mode] = {k: float(np.median([x[k] for x in r])) for k in r[0] if k != 'maps'}
    summary['speedup_scene_to_ply'] = summary['two_step']['scene_to_ply_s'] / summary['in_run']['scene_to_ply_s']
    print(json.dumps({k: v for k, v in summary.items() if k != 'runs'}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)
    if not same:
        raise SystemExit('the two pipelines wrote different point coordinates')


if __name__ == '__main__':
    main()
