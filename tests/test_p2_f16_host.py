"""No GPU: the host side of the one-term ("f16") mode of the perceptual loss's p2 convolutions -- the tuning-key table (key name
<-> VUNET_TUNE_* value <-> header), ``set_p2_precision``'s argument checking and what it selects, the trainers' config default."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_keys():
    txt = open(os.path.join(ROOT, "include", "vunet_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define VUNET_TUNE_(\w+) (\d+)\s*$", txt, flags=re.M)}


def test_tuning_key_table_matches_the_header():
    from behavior_driven_video_synthesis_amd import ops
    hdr = _header_keys()
    count = hdr.pop("COUNT")
    assert hdr["P2_TERMS"] == 9 and count == 10
    assert sorted(hdr.values()) == list(range(count))                          # dense, no value twice
    assert {k.lower(): v for k, v in hdr.items()} == ops._TUNING_KEYS            # name <-> value, both ways
    # the library takes every key of the table and refuses the first one past it
    from behavior_driven_video_synthesis_amd import _lib
    lib = _lib.lib()
    try:
        for v in ops._TUNING_KEYS.values():
            assert lib.vunet_set_tuning(v, 0) == 0
        assert lib.vunet_set_tuning(count, 0) != 0
        with pytest.raises(KeyError):
            ops.set_tuning("p2_precision", 1)
        with pytest.raises(KeyError):
            ops.tuning("p2_precision")
    finally:
        ops.set_tuning("p2_terms", 0)


def _variant(ops, n, c, h, w, m):
    d = ops.P2Desc(n, c, h, w, m, 0)
    buf = ctypes.create_string_buffer(96)
    ops._call("vunet_p2_conv_variant", ctypes.byref(d), buf, 96)
    return buf.value.decode()


def test_set_p2_precision_checks_its_argument_and_selects_the_one_term_kernels():
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    assert ip.p2_precision() == "split"
    for bad in ("bf16", "fp16", "F16", "", None, 1):
        with pytest.raises(ValueError):
            ip.set_p2_precision(bad)
    assert ip.p2_precision() == "split"                                          # a refused call changes nothing
    two = {"conv1_2": "conv_p2_kernel<4, 32, 1>", "conv4_x": "conv_p2a_kernel<32>", "conv5_x": "conv_p2_kernel<4, 16, 1>"}
    one = {"conv1_2": "conv_p2_kernel<4, 32, 1, 1>", "conv4_x": "conv_p2a_kernel<32, 1>", "conv5_x": "conv_p2_kernel<4, 16, 1, 1>"}
    geo = {"conv1_2": (16, 64, 256, 256, 64), "conv4_x": (16, 512, 32, 32, 512), "conv5_x": (16, 512, 16, 16, 512)}
    try:
        assert {k: _variant(ops, *g) for k, g in geo.items()} == two
        assert ip.set_p2_precision("f16") == "split"                            # returns the previous mode
        assert ip.p2_precision() == "f16" and ops.tuning("p2_terms") == 1
        assert {k: _variant(ops, *g) for k, g in geo.items()} == one             # distinct names, rocprofv3's spelling
        ops.set_tuning("p2_form", 3)                                             # no lockstep one-term kernel: the antiphase one
        assert _variant(ops, *geo["conv4_x"]) == one["conv4_x"]
        ops.set_tuning("p2_form", 0)
        assert ip.set_p2_precision("f16") == "f16"
        assert ip.set_p2_precision("split") == "f16"
        assert ip.p2_precision() == "split" and {k: _variant(ops, *g) for k, g in geo.items()} == two
        ops.set_tuning("p2_terms", 2)                                            # 2 names the default as well
        assert ip.p2_precision() == "split" and {k: _variant(ops, *g) for k, g in geo.items()} == two
    finally:
        ops.set_tuning("p2_form", 0)
        ops.set_tuning("p2_terms", 0)


def test_env_tuning_selects_the_mode(monkeypatch):
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    monkeypatch.setenv("VUNET_TUNING", "p2_terms=1")
    try:
        ops.apply_env_tuning()
        assert ip.p2_precision() == "f16"
        # a trainer whose config is silent leaves the process's mode alone; one that names a mode selects it
        assert ip.apply_config_precision({}) == "split" and ip.p2_precision() == "f16"
        assert ip.apply_config_precision({"vgg_precision": "split"}) == "split" and ip.p2_precision() == "split"
    finally:
        ops.set_tuning("p2_terms", 0)


def test_trainers_read_vgg_precision_with_the_default_split():
    import copy
    from behavior_driven_video_synthesis_amd.experiments import shape_and_pose_net as spn, vunet as vn
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    for mod in (spn, vn):
        assert "vgg_precision" not in mod.DEFAULT_CONFIG["training"]            # absent = "split"
        assert ip.vgg_precision_from_config(mod.DEFAULT_CONFIG["training"]) == "split"
        assert mod.apply_config_precision is ip.apply_config_precision          # what the constructor calls
    assert ip.vgg_precision_from_config({"vgg_precision": "f16"}) == "f16"
    with pytest.raises(ValueError, match="vgg_precision"):
        ip.vgg_precision_from_config({"vgg_precision": "half"})
    # a ShapePoseNet built on the CPU from the default config, and from one that names a mode
    cfg = copy.deepcopy(spn.DEFAULT_CONFIG)
    cfg["data"]["spatial_size"] = 32
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(train_regressor=False)
    try:
        tr = spn.ShapePoseNet(cfg, device="cpu", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
        assert tr.vgg_precision == "split" and ip.p2_precision() == "split"
        cfg["training"]["vgg_precision"] = "f16"
        tr = spn.ShapePoseNet(cfg, device="cpu", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
        assert tr.vgg_precision == "f16" and ip.p2_precision() == "f16"
        cfg["training"]["vgg_precision"] = "fp16"
        with pytest.raises(ValueError, match="vgg_precision"):
            spn.ShapePoseNet(cfg, device="cpu", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    finally:
        ip.set_p2_precision("split")
