"""Host side of the flow's bf16 weight mode (include/vunet_seq_bf16.h, seq.py): what can be checked without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_an_unknown_weight_precision_is_refused_before_any_device_work():
    from behavior_driven_video_synthesis_amd.models.flow.simple_flow import UnsupervisedTransformer2
    flow = UnsupervisedTransformer2(flow_in_channels=8, flow_mid_channels=16, flow_hidden_depth=1, n_flows=1)   # on the CPU
    for bad in ("fp8", "BF16", "", None):
        with pytest.raises(ValueError, match="weight precision"):
            flow.set_weight_precision(bad)
    assert flow.flow.weight_precision == "f32" and flow.flow._engine is None
    # a valid mode is recorded on the module (no engine, no images yet) and the previous one is returned
    assert flow.set_weight_precision("bf16") == "f32"
    assert flow.flow.weight_precision == "bf16" and flow.flow._engine is None
    assert flow.set_weight_precision("f32") == "bf16"


def test_the_training_engine_is_refused_in_bf16_mode_on_the_host():
    from behavior_driven_video_synthesis_amd.models.flow.simple_flow import UnsupervisedTransformer2
    flow = UnsupervisedTransformer2(flow_in_channels=8, flow_mid_channels=16, flow_hidden_depth=1, n_flows=1)
    flow.set_weight_precision("bf16")
    with pytest.raises(RuntimeError, match="bf16 images are for inference only"):
        flow.flow.train_engine()


def test_ctypes_argument_lists_match_the_prototypes_of_the_header():
    """The two entry points as seq.py calls them, against the prototypes parsed from include/vunet_seq_bf16.h itself."""
    from behavior_driven_video_synthesis_amd import _lib
    txt = open(os.path.join(ROOT, "include", "vunet_seq_bf16.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
              for m in re.finditer(r"\bint\s+(vunet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt, flags=re.S)}
    assert sorted(protos) == ["vunet_seq_linear_bf16w", "vunet_seq_pack_tiles_bf16"]
    P, I = ctypes.c_void_p, ctypes.c_int32
    # what seq.tile_image_bf16 / seq.linear_bf16w pass, in order
    want = {"vunet_seq_pack_tiles_bf16": [("w", P), ("ld", I), ("M", I), ("K", I), ("wt16", P), ("stream", P)],
            "vunet_seq_linear_bf16w": [("d", P), ("layout", I), ("w0", P), ("w1", P), ("x", P), ("bias0", P), ("bias1", P), ("y", P),
                                       ("stream", P)]}
    declared = _lib.declared_prototypes()
    for name, args in want.items():
        assert [a.replace("*", " ").split()[-1] for a in protos[name]] == [n for n, _ in args], name
        assert [P if "*" in a else I for a in protos[name]] == [t for _, t in args], name
        assert all("*" in a or a.split()[0] == "int32_t" for a in protos[name]), name
        assert declared[name] == [t for _, t in args], name
    assert "vunet_seq_pack_tiles_bf16" in _lib.declared_symbols() and "vunet_seq_linear_bf16w" in _lib.declared_symbols()
