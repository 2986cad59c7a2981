"""ops.py was split by concern (_hipcall: call plumbing, evaluation, sheets); everything it offered before is still an
attribute of ``ops``, and what moved is the same object in both places.  Needs no GPU and no library."""
from tiaozhanbei_unet_amd import _hipcall, evaluation, ops, sheets

# every name without a leading underscore that ops.py defined (def, class or assignment at module level) before the split
PUBLIC = (
    "BN_EPS", "register_grad_slots", "unregister_grad_slots", "release_grad_slot", "grad_out", "PackInput",
    "to_operator_layout", "narrow_channels", "seg_cols", "seg_col", "pack_weight", "PackCache", "set_active_packs",
    "packed", "GradSink", "SHARE_SKIP_GRADS", "share_grad", "FOLD_EVAL_BN", "parameters_written", "FUSE_BN_BWD",
    "FUSE_BN_HEAD", "FUSE_BN_POOL", "FUSE_BN_CONVT", "BnLink", "ConvBnRelu", "FirstConvBnRelu", "FIRST_LAYER_KERNELS",
    "FUSE_FIRST_BN_BWD", "first_layer_ok", "ChannelDropout", "anomaly_score", "MaxPool2", "ConvT2x2", "Bilinear2x", "Head",
    "MseFocal", "Ssim", "threshold_confusion", "BinaryAUC", "label_regions", "RegionOverlapAUC", "label_class_regions",
    "RECORD_FIELDS", "ClassRegionMatcher", "preprocess_u8", "IMAGENET_MEAN", "IMAGENET_STD", "MAX_PANELS", "colormap_lut",
    "panel_range", "render_sheet", "TAB10", "seg_confidence", "class_palette", "viridis_lut", "render_seg_sheet",
    "prof_enable", "prof_collect", "prof_kernels", "adam_step_")
# its module aliases and private plumbing that model.py, augment.py, metrics.py, bench.py, the tools and the tests reach
PLUMBING = ("L", "C", "torch", "_DT", "_ptr", "_stream", "_require_cuda", "_nhwc_empty", "_is_nhwc", "_as_nhwc",
            "_workspace", "_views", "_pad64")
# what the tests and model.py patch or read through the ops namespace stays DEFINED there
STATE = ("_train_generation", "_write_generation", "_active_packs", "_folded", "_narrow_views", "_grad_slots",
         "_grad_taken", "SHARE_SKIP_GRADS", "FOLD_EVAL_BN", "FUSE_BN_BWD", "FUSE_BN_HEAD", "FUSE_BN_POOL", "FUSE_BN_CONVT",
         "FIRST_LAYER_KERNELS", "FUSE_FIRST_BN_BWD", "pack_weight", "packed", "PackCache", "parameters_written")

MOVED = {
    evaluation: ("anomaly_score", "threshold_confusion", "BinaryAUC", "label_regions", "RegionOverlapAUC",
                 "label_class_regions", "RECORD_FIELDS", "ClassRegionMatcher", "preprocess_u8"),
    sheets: ("IMAGENET_MEAN", "IMAGENET_STD", "MAX_PANELS", "colormap_lut", "panel_range", "render_sheet", "TAB10",
             "seg_confidence", "class_palette", "viridis_lut", "render_seg_sheet"),
    _hipcall: ("BN_EPS", "prof_enable", "prof_collect", "prof_kernels") + PLUMBING[3:],
}


def test_every_public_name_of_ops_is_still_there():
    missing = [n for n in PUBLIC + PLUMBING + STATE if not hasattr(ops, n)]
    assert not missing, missing


def test_moved_names_are_the_same_objects_in_their_new_homes():
    for home, names in MOVED.items():
        for n in names:
            assert getattr(ops, n) is getattr(home, n), (home.__name__, n)
    assert ops._workspace is _hipcall._workspace


def test_state_and_switches_live_in_ops_itself():
    for n in STATE:
        for other in (_hipcall, evaluation, sheets):
            assert not hasattr(other, n), (other.__name__, n)
        v = getattr(ops, n)
        if callable(v):
            assert v.__module__ == ops.__name__, n
    moved = {n for names in MOVED.values() for n in names}
    assert not moved & set(STATE)


def test_private_helpers_of_the_moved_families_are_not_re_exported():
    for n in ("_select_runs", "_image_planes", "_class_maps", "_class_regions_error", "_luts", "_seg_tables", "_panels",
              "_seg_panels", "_workspaces"):
        assert not hasattr(ops, n), n
    assert hasattr(evaluation, "_select_runs") and hasattr(sheets, "_luts") and hasattr(_hipcall, "_workspaces")
