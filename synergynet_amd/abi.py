"""ctypes binding of the C ABI in include/synergy_hip.h (libsynergy_hip.so).

There is no CPU fallback: if the HIP library is missing or a call fails this raises.
torch is imported first on purpose so that the library's libamdhip64.so.7 dependency
resolves to the HIP runtime torch already loaded (one runtime per process; device
pointers and streams are shared with torch).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede loading the library, see module docstring)

from .build import LIB

SYN_ERR_INVALID, SYN_ERR_NOT_LOADED = -1, -3
SYN_ERR_PARAM_LEN = -4
SYN_DETECT_BATCH_MAX_FRAMES = 1024          # include/synergy_hip.h: syn_detect_batch refuses a larger N
SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES = 163776 # include/synergy_hip.h: syn_train_transform_u8 refuses a face of more bytes (3 H W)
_lib = None


class SynergyHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libsynergy_hip: {msg} (status {code})')
        self.code = code
        self.msg = msg


_SIGS = {
    'syn_last_error': (C.c_char_p, []),
    'syn_abi_version': (C.c_int, []),
    'syn_create': (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    'syn_destroy': (C.c_int, [C.c_void_p]),
    'syn_backbone_flat_count': (C.c_size_t, []),
    'syn_load_backbone': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_numerics_report': (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    'syn_set_schedule': (C.c_int, [C.c_void_p, C.c_int]),
    'syn_backbone_range_status': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    'syn_backbone_range_events': (C.c_int, [C.c_void_p]),
    'syn_backbone_calibrate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    'syn_resnet50_flat_count': (C.c_size_t, []),
    'syn_load_backbone_resnet50': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_resnet50_flops_per_face': (C.c_double, []),
    'syn_mobilenet1_flat_count': (C.c_size_t, [C.c_int]),
    'syn_mobilenet1_flops_per_face': (C.c_double, [C.c_int]),
    'syn_load_backbone_mobilenet1': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    'syn_ghostnet_flat_count': (C.c_size_t, []),
    'syn_ghostnet_flops_per_face': (C.c_double, []),
    'syn_load_backbone_ghostnet': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_resnest50_flat_count': (C.c_size_t, []),
    'syn_resnest50_flops_per_face': (C.c_double, []),
    'syn_load_backbone_resnest50': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_resnet_basic_flat_count': (C.c_size_t, [C.c_int]),
    'syn_resnet_basic_flops_per_face': (C.c_double, [C.c_int]),
    'syn_load_backbone_resnet_basic': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    'syn_load_basis': (C.c_int, [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_int]),
    'syn_constants_bytes': (C.c_size_t, [C.c_void_p]),
    'syn_export_constants': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'syn_import_constants': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'syn_bcast_constants': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'syn_describe_constants': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_pack_constants_host_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'syn_pack_constants_host': (C.c_int, [C.c_int, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    'syn_check_constants_host': (C.c_int, [C.c_void_p, C.c_size_t]),
    'syn_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int]),
    'syn_backbone_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_backbone_forward_u8': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_crop_resize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]),
    'syn_crop_resize_frames': (C.c_int, [C.c_void_p] * 11 + [C.c_int, C.c_void_p]),
    'syn_lanczos4_tables': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_face_tables': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p]),
    'syn_compact_detections': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    'syn_detector_flat_count': (C.c_size_t, []),
    'syn_load_detector': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_detector_prior_count': (C.c_int, [C.c_int, C.c_int]),
    'syn_detect': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                             C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    'syn_detect_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_nme': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'syn_load_triangles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    'syn_mesh_shade': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_rasterize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'syn_add_weighted': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    'syn_load_uv_map': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    'syn_select_topology': (C.c_int, [C.c_void_p, C.c_int]),
    'syn_uv_colors': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_gather_vertices': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_mesh_shade_textured': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    'syn_rasterize_triangles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'syn_vertex_visibility': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_sample_vertex_colors': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    'syn_uv_scatter': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'syn_texture_fill': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_load_tex_coords': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'syn_render_texture': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'syn_reconstruct': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_reconstruct_pitched': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'syn_pose': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_landmarks_pose': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_pose_matrix': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_synergy_flat_count': (C.c_size_t, []),
    'syn_synergy_folded_count': (C.c_size_t, []),
    'syn_fold_synergy_host': (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    'syn_load_synergy': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'syn_refine_landmarks': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_refine_points': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_landmarks_to_param': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_wing_loss': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'syn_param_loss': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_synergy_losses': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_synergy_losses_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    'syn_synergy_losses_backward_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_update_synergy_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'syn_synergy_bn_channels': (C.c_size_t, []),
    'syn_synergy_losses_train': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_float, C.c_void_p]),
    'syn_export_synergy_flat': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'syn_wing_loss_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    'syn_param_loss_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_center_crop_u8': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'syn_train_transform_u8': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_backbone_launch_count': (C.c_int, [C.c_void_p]),
    'syn_backbone_profile': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'syn_mobilenet1_layer': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    'syn_mobilenet2_span': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    'syn_resnet50_span': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    # block 0..15 bottlenecks, 16 ConvBnAct, 17 pool + conv_head + heads, 18 conv_stem (in = normalised fp32 crops NCHW, no aux)
    'syn_ghostnet_block': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    'syn_resnest50_block': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    'syn_resnet_basic_block': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    'syn_reconstruct_profile': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'syn_backbone_flops_per_face': (C.c_double, []),
    'syn_pointwise_flops_per_face': (C.c_double, []),
}

EXPORTED_SYMBOLS = tuple(_SIGS)          # exactly the symbols include/synergy_hip.h declares
# test hook exported by the library but deliberately not part of the public header
_SIGS = dict(_SIGS, syn_debug_feature=(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
             syn_debug_profile_block=(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
             syn_debug_detect_raw=(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 5),
             syn_debug_poison_workspace=(C.c_int, [C.c_void_p, C.c_int, C.c_int]),
             syn_debug_resnet_pairs=(C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]),
             syn_debug_det_select_nms=(C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
             syn_debug_det_preproc=(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]))


def lib():
    """The loaded library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        path = os.environ.get('SYNERGY_HIP_LIB', LIB)      # A/B of two builds on one box (tools/ab_bench.sh); default: the in-tree build
        if not os.path.isfile(path):
            raise SynergyHipError(-100, f'{path} not built; run `python -c "import __graft_entry__ as g; g.build()"`')
        l = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().syn_last_error().decode(errors='replace')
        raise SynergyHipError(rc, msg)
