"""mesh_fusion's command with the consistency mask and the view weights: the written depth maps of a scene
are meshed from the depths that the fusion's num_consistent other views agree on (--consistent), each view weighted per pixel by
its agreement count or by the probability map (--weights agree|prob).  Every option of mesh_fusion, and four more; mesh_fusion's own
command line and the ETH3D driver's keep the options they had (the driver takes consistent= and weights= in run_eval_pc's mesh dict).

    python -m atvsnet_amd.atvsnet.mesh_consistent --maps <out>/<scene> --voxel V --out mesh.ply
        [--consistent [--disp_threshold 0.01 --num_consistent 2]] [--weights agree|prob] [every option of mesh_fusion]

The cameras are packed with depth_fusion.projection_matrix / pack_cameras and the slab carries the fake normal, under which the
normal test rejects nothing (mesh_fusion.support_of_maps).  --weights prob needs the probability files.  This module imports without
a GPU."""
from . import mesh_fusion


def make_parser():
    parser = mesh_fusion.make_parser()
    parser.description = parser.description + '; from consistency-masked depths (--consistent) and with per-pixel view weights (--weights)'
    mesh_fusion.add_support_options(parser)
    return parser


def cli(argv=None):
    return mesh_fusion.cli(argv, make_parser())


if __name__ == '__main__':
    cli()
