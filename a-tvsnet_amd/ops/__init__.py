"""Python face of the C-ABI (include/atvsnet_hip.h): one function per entry point, in these modules --

    base      ctypes plumbing, the dispatch switches (`cfg`, `configure`), launch timing
    packing   weights in operand order + their cache, tap lists, the chunk-planar layout
    geometry  homographies, warps, cost / refinement volumes, soft-argmin
    norm      batch norm, element-wise glue, the deferred batch-norm algebra (PendingBN / PendingSum / LazySlice)
    launch    dispatch policy (`conv_plan`, the `*_ok` predicates) and single-kernel launch wrappers
    convolution  `conv()` and the composite forms (SplitVolume, siblings, stems, transposed convolution)
    aanet     AANet aggregation, depth-map fusion
    prepare   the scene driver's view preparation (uint8 image -> network input, 1/4 image)
    colmap    COLMAP model import: per-image depth range, co-visibility matrix; undistortion: sampling map, image gather
    cloud     point-cloud scoring: uniform grid, exact nearest neighbour within a radius, tolerance counts;
              registration: transform, pair moments, voxel down-sampling; neighbourhoods: k nearest neighbours, radius counts,
              outlier statistics, bounding box, normals by PCA over the k nearest; rendering: a scan splatted into cameras as nearest-depth maps; ETH3D-style
              scoring: a point's free-space excess against scanner cube maps, voxel-averaged shares
    tsdf      a surface from depth maps: a block-sparse TSDF volume integrated from them, a marching-tetrahedra mesh of it
    mesh      a triangle mesh rendered into cameras (nearest depth and face per pixel), depth maps occluded by such a rendering
    mesh_topology  a mesh's connected components, a selection of its faces with the vertices compacted, its edge census
    mesh_simplify  vertex clustering: the clusters' exact sums and fixed-point quadrics, the representatives, the rewritten faces
    mesh_sample    a mesh's surface sampled uniformly by area: per-face counts by stochastic rounding, the samples' points, colours, normals
    mesh_distance  exact point-to-triangle distances from a cloud to a mesh: a uniform grid of face references, the nearest face within a radius
    mesh_smooth    Taubin smoothing: the vertices' distinct neighbours, positions as integers, the umbrella step as an exact gather;
              area-weighted vertex normals

Every name is re-exported here (`ops.conv`, `ops.cfg`, ...): callers import this package, never a submodule.  The modules share
ONE set of state objects (`cfg`, the pack caches, the timing watch), defined once in base / packing and imported by reference.
"""
from .base import (Config, Stats, _ERR, _Timed, _call, _dev_ok, _new, _p, _ptr_array, _side_pool, _side_stream, _size, _stats,
    _stats_buffer, _stream, _watch, _watched, cfg, configure, launches, watch)      # noqa: F401
from .packing import (PLANAR_PAD, _Packed, _abi_pack, _fold_cache, _pack_cache, _virt_cache, _xkind, _xp_cache, cache_snapshot,
    clear_pack_cache, conv_taps, deconv_s2_class_taps, deconv_up_ok, invalidate_weights, pack_conv3d_b, pack_conv_c16,
    pack_conv_c16b, pack_conv_weights, pack_conv_weights_tiled, pack_conv_xp, pack_conv_xp_sibling, pack_deconv_up,
    planar_cost_volume_ok, planar_pieces_decode, planar_pieces_ok, planar_stride, planar_view, same_pad, split_on)      # noqa: F401
from .geometry import (WARP_NEAREST, absdiff_mask, build_cost_volume, geo_ref_planes, geo_volume, get_homographies,
    interpolate, pixel_grids, probability_map, softargmin, tile_planes, transform_depth, transform_depth_batch,
    upsample_softargmin, visual_hull, warp_by_depth, warp_by_depth_err, warp_planes)      # noqa: F401
from .norm import (LAZY, LazySlice, PendingBN, PendingSum, _flag_pool, _param_groups, add_n, avg_pool_same, batch_norm,
    bn_add, bn_apply, bn_params, channel_stats, concat_channels, copy_channels, nonfinite_flag, nonfinite_seen,
    resize_bilinear, siblings_prologue_ok, stack)      # noqa: F401
from .launch import (ConvPlan, Fin, XPAIR_TAPS, _fin_counter, _fin_pool, _from5, _pick_tile_m, _to5,
    _xpair_virtual_kernel, bottleneck, bottleneck_ok, conv1x1, conv1x1_ok, conv2d_lds, conv2d_lds_ok, conv2d_tail,
    conv2d_tail_ok, conv_blocks, conv_geometry, conv_launch, conv_plan, conv_tiled_launch, conv_xp_launch, norm_on_load_2d_ok,
    norm_on_load_3d_ok, pack_conv1x1, pack_conv2d_lds, tiled_blocks, tiled_nsplit, tiled_tile_y, xp_blocks)      # noqa: F401
from .convolution import (SplitVolume, _DECONV_OFFSETS, _deconv_virtual_kernel, _fold_split_weights, conv, conv3d_8to1,
    conv3d_transpose_s2, conv_siblings, conv_split, conv_split_into_plane, conv_split_siblings, deconv_sum_ok,
    photo_pieces_ok, planar_concat_ok, refine_stems, siblings_ok)      # noqa: F401
from .prepare import (ViewPlan, prepare_taps, prepare_view, prepare_workspace, resize_u8_host, view_plan)      # noqa: F401
from .aanet import (aanet_combine, aanet_fused, aanet_fused_ok, aanet_partial, depth_normals, divide, fusibile,
    fusibile_scene, fusion_stage, fusion_support)      # noqa: F401
from .colmap import COVIS_MAX_IMAGES, colmap_covisibility, colmap_depth_range      # noqa: F401
from .colmap import UNDISTORT_MAX_SIDE, UNDISTORT_MODELS, undistort_map, undistort_remap      # noqa: F401
from .cloud import CLOUD_MAX_POINTS, CLOUD_MAX_TOLERANCES, CloudGrid, cloud_counts, cloud_grid, cloud_nearest      # noqa: F401
from .cloud import cloud_bounds, cloud_pair_moments, cloud_plane_moments, cloud_transform, cloud_voxel_downsample      # noqa: F401
from .cloud import CLOUD_MAX_K, cloud_knn, cloud_knn_mean, cloud_radius_count, cloud_sor_stats      # noqa: F401
from .cloud import cloud_normals, cloud_plane_moments_target      # noqa: F401
from .cloud import cloud_feature_nearest, cloud_fpfh, cloud_ransac      # noqa: F401
from .cloud import SCAN_RENDER_MAX_CAMS, SCAN_RENDER_MAX_SPLAT, scan_render      # noqa: F401
from .cloud import CLOUD_SCAN_MAX_WINDOW, cloud_scan_excess, cloud_voxel_shares      # noqa: F401
from .tsdf import TSDF_MAX_DIRECTORY, TSDF_MAX_MESH_BLOCKS, TSDF_MAX_PIXEL_BLOCKS, TsdfVolume, tsdf_free_views, tsdf_integrate, tsdf_mesh      # noqa: F401
from .mesh import MESH_RENDER_SMALL_PIXELS, depth_occlude, mesh_render      # noqa: F401
from .mesh_topology import (MESH_CENSUS_MIN_SLOTS, MESH_CENSUS_WORDS, MESH_TOPOLOGY_MAX_FACES, mesh_components, mesh_edge_census,
    mesh_select)      # noqa: F401
from .mesh_simplify import (MESH_PLACEMENTS, MESH_RANK_EPSILON, MESH_SIMPLIFY_MIN_SLOTS, MESH_SIMPLIFY_SOLVE_UNITS, MeshClusters,
    mesh_cluster, mesh_cluster_faces, mesh_cluster_max_move, mesh_cluster_place, mesh_cluster_quadrics)      # noqa: F401
from .mesh_sample import MESH_SAMPLE_MAX, MeshSamples, mesh_sample, mesh_sample_counts, mesh_sample_points      # noqa: F401
from .mesh_distance import MESH_GRID_MAX_REFS, MeshGrid, mesh_grid, mesh_nearest      # noqa: F401
from .mesh_smooth import (MESH_ADJACENCY_INFO, MESH_ADJACENCY_MIN_SLOTS, MESH_FLAG_BOUNDARY, MESH_FLAG_FINITE, MESH_FLAG_NONMANIFOLD,
    MESH_SMOOTH_LAMBDA, MESH_SMOOTH_MAX_ITERATIONS, MESH_SMOOTH_MU, MeshAdjacency, mesh_adjacency, mesh_dequantize, mesh_face_extent,
    mesh_normals_from_sums, mesh_quantize, mesh_smooth, mesh_smooth_lattice, mesh_smooth_pass, mesh_vertex_normal_sums,
    mesh_vertex_normals)      # noqa: F401
from .. import _lib      # noqa: F401  (ops._lib: tests and tools reach the loader through this package)
