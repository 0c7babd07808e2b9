#!/usr/bin/env python
"""Import a COLMAP reconstruction as a scene of the drivers (atvsnet/colmap.py).

    python -m atvsnet_amd.atvsnet.colmap_scene --dense_folder <colmap dense dir> --out <data_root>/eth3d/<scene> \\
           [--max_d 128] [--num_neighbors 10] [--percentile 0.99] [--stretch 1.33333] [--link]
    python -m atvsnet_amd.atvsnet.eval_pointcloud --data_root <data_root> --scenes <scene> --scene_cache --fuse ...

<dense_folder> is the output of `colmap image_undistorter` (sparse/ + images/).  Depth ranges and co-visibility run on the GPU.
"""
from __future__ import print_function

import argparse
import time


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dense_folder', required=True, help='sparse/ (text or binary model) and images/ of colmap image_undistorter')
    ap.add_argument('--out', required=True, help='scene folder to write (e.g. <data_root>/eth3d/<scene>)')
    ap.add_argument('--max_d', type=int, default=128, help='depth planes written into each camera (the driver sweeps its own --max_d)')
    ap.add_argument('--num_neighbors', type=int, default=10, help='source views listed per reference in pair.txt')
    ap.add_argument('--percentile', type=float, default=0.99, help='disparity quantiles p and 1 - p give the depth range')
    ap.add_argument('--stretch', type=float, default=1.33333, help='the range is widened by this factor on both ends')
    ap.add_argument('--link', action='store_true', help='symlink the undistorted JPEGs instead of copying them')
    ap.add_argument('--gpu_id', type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    from . import colmap
    torch.cuda.set_device(a.gpu_id)
    t0 = time.time()
    r = colmap.make_scene(a.dense_folder, a.out, max_d=a.max_d, num_neighbors=a.num_neighbors, percentile=a.percentile,
                          stretch=a.stretch, link=a.link)
    m = r['model']
    print('colmap import: %d images (%d left out), %d points, %d observations -> %s in %.2f s' %
          (len(m.image_ids), len(r['skipped']), len(m.xyz), int(m.offsets[-1]), a.out, time.time() - t0))
    return r


if __name__ == '__main__':
    main()
