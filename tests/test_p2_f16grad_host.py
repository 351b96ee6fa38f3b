"""No GPU: the host side of the "f16grad" mode of the perceptual loss's p2 convolutions (tuning value ``p2_terms`` = 3: one
product per tap in the DATA-GRADIENT launches only, the forward launches exactly as in "split") -- the public switch, what the
variant query reports for forward (``relu`` = 1) and data-gradient (``relu`` = 0) descriptors, the environment spelling and the
trainers' config key.  Data gradients run the four-wave one-term kernel; with at most 256 workgroups (one per CU) its
two-x-buffer instantiation ``conv_p2_kernel<4, CT, 2, 1>``."""
import copy
import ctypes

import pytest

# the VGG19 geometries of the bs-16 256 x 256 step: (N, C, H, W, M)
GEO = {"conv1_2": (16, 64, 256, 256, 64), "conv2_2": (16, 128, 128, 128, 128), "conv3_x": (16, 256, 64, 64, 256),
       "conv4_x": (16, 512, 32, 32, 512), "conv5_x": (16, 512, 16, 16, 512)}
TWO = {"conv1_2": "conv_p2_kernel<4, 32, 1>", "conv2_2": "conv_p2a_kernel<32>", "conv3_x": "conv_p2a_kernel<32>",
       "conv4_x": "conv_p2a_kernel<32>", "conv5_x": "conv_p2_kernel<4, 16, 1>"}
ONE = {"conv1_2": "conv_p2_kernel<4, 32, 1, 1>", "conv2_2": "conv_p2a_kernel<32, 1>", "conv3_x": "conv_p2a_kernel<32, 1>",
       "conv4_x": "conv_p2a_kernel<32, 1>", "conv5_x": "conv_p2_kernel<4, 16, 1, 1>"}
# "f16grad", data gradient: four waves everywhere unless p2_form asks for the antiphase kernel; conv5_x has 16 x 2 x 1 x 8 = 256
# workgroups: two x buffers.  p2_form = 1: the single-buffer kernel everywhere
GRAD = {"conv1_2": "conv_p2_kernel<4, 32, 1, 1>", "conv2_2": "conv_p2_kernel<4, 32, 1, 1>", "conv3_x": "conv_p2_kernel<4, 32, 1, 1>",
        "conv4_x": "conv_p2_kernel<4, 32, 1, 1>", "conv5_x": "conv_p2_kernel<4, 16, 2, 1>"}
GRAD_FOUR = dict(GRAD, conv5_x="conv_p2_kernel<4, 16, 1, 1>")
GRAD_WIDE = {"conv1_2": "conv_p2_kernel<4, 32, 1, 1>", "conv2_2": "conv_p2a_kernel<32, 1>", "conv3_x": "conv_p2a_kernel<32, 1>",
             "conv4_x": "conv_p2a_kernel<32, 1>", "conv5_x": "conv_p2a_kernel<16, 1>"}      # (conv1_2: M = 64, four waves only)


@pytest.fixture(autouse=True)
def _restore_the_dispatcher():
    yield
    from behavior_driven_video_synthesis_amd import ops
    ops.set_tuning("p2_terms", 0)
    ops.set_tuning("p2_form", 0)


def _variant(ops, n, c, h, w, m, relu):
    d = ops.P2Desc(n, c, h, w, m, relu)
    buf = ctypes.create_string_buffer(96)
    ops._call("vunet_p2_conv_variant", ctypes.byref(d), buf, 96)
    return buf.value.decode()


def _names(ops, relu):
    return {k: _variant(ops, *g, relu) for k, g in GEO.items()}


def test_the_switch_selects_value_3_and_leaves_the_other_modes_as_they_were():
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    assert ip.P2_PRECISIONS == ("split", "f16", "f16grad")
    assert ip.p2_precision() == "split"
    assert ip.set_p2_precision("f16grad") == "split"                             # returns the previous mode
    assert ip.p2_precision() == "f16grad" and ops.tuning("p2_terms") == 3
    for bad in ("f16_grad", "F16GRAD", "grad", "", None, 3):
        with pytest.raises(ValueError, match="f16grad"):                         # (the message lists the modes)
            ip.set_p2_precision(bad)
        assert ip.p2_precision() == "f16grad" and ops.tuning("p2_terms") == 3    # a refused call changes nothing
    assert ip.set_p2_precision("f16grad") == "f16grad"
    assert ip.set_p2_precision("f16") == "f16grad"
    assert ip.p2_precision() == "f16" and ops.tuning("p2_terms") == 1
    assert _names(ops, 0) == ONE and _names(ops, 1) == ONE                       # "f16": every launch, the two-term form rule
    assert ip.set_p2_precision("split") == "f16"
    assert ip.p2_precision() == "split" and ops.tuning("p2_terms") == 0
    assert _names(ops, 0) == TWO and _names(ops, 1) == TWO
    assert ip.set_p2_precision("f16grad") == "split"
    assert ip.set_p2_precision("split") == "f16grad"


def test_variant_query_in_f16grad_mode():
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    split_fwd = _names(ops, 1)
    assert split_fwd == TWO
    ip.set_p2_precision("f16grad")
    assert _names(ops, 1) == split_fwd                                           # forward launches: the "split" kernels
    assert _names(ops, 0) == GRAD                                                # data gradients: one term, four waves
    # the two-buffer kernel up to 256 workgroups and not beyond: conv4_1's data gradient (512 -> 256 channels) has 16 x 4 x 1 x 4
    assert _variant(ops, 16, 512, 32, 32, 256, 0) == "conv_p2_kernel<4, 32, 2, 1>"
    assert _variant(ops, 17, 512, 32, 32, 256, 0) == "conv_p2_kernel<4, 32, 1, 1>"
    assert _variant(ops, 16, 512, 32, 32, 256, 1) == "conv_p2_kernel<4, 32, 1>"
    for form, fwd, grad in ((1, {k: f"conv_p2_kernel<4, {16 if g[3] == 16 else 32}, 1>" for k, g in GEO.items()}, GRAD_FOUR),
                            (2, {k: ("conv_p2_kernel<4, 32, 1>" if g[4] % 128 else f"conv_p2a_kernel<{16 if g[3] == 16 else 32}>")
                                 for k, g in GEO.items()}, GRAD_WIDE)):
        ops.set_tuning("p2_form", form)
        assert _names(ops, 1) == fwd, form                                        # (the forward follows p2_form as in "split")
        assert _names(ops, 0) == grad, form
    ops.set_tuning("p2_form", 3)                                                 # no lockstep one-term kernel: the antiphase one
    assert _names(ops, 0) == GRAD_WIDE
    assert _variant(ops, *GEO["conv4_x"], 1) == "conv_p2_kernel<8, 32, 2>"       # ... while the forward runs the lockstep two-term one
    ops.set_tuning("p2_form", 0)
    ip.set_p2_precision("split")
    assert _names(ops, 0) == TWO


def test_env_tuning_and_config_select_the_mode(monkeypatch):
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments import shape_and_pose_net as spn
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    monkeypatch.setenv("VUNET_TUNING", "p2_terms=3")
    ops.apply_env_tuning()
    assert ip.p2_precision() == "f16grad"
    assert ip.apply_config_precision({}) == "split" and ip.p2_precision() == "f16grad"      # a silent config leaves the mode alone
    assert ip.apply_config_precision({"vgg_precision": "split"}) == "split" and ip.p2_precision() == "split"
    assert ip.vgg_precision_from_config({"vgg_precision": "f16grad"}) == "f16grad"
    with pytest.raises(ValueError, match="f16grad"):
        ip.vgg_precision_from_config({"vgg_precision": "f16-grad"})
    assert ip.apply_config_precision({"vgg_precision": "f16grad"}) == "f16grad" and ops.tuning("p2_terms") == 3
    ip.set_p2_precision("split")
    # a ShapePoseNet built on the CPU from a config that names the mode
    cfg = copy.deepcopy(spn.DEFAULT_CONFIG)
    cfg["data"]["spatial_size"] = 32
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(train_regressor=False, vgg_precision="f16grad")
    tr = spn.ShapePoseNet(cfg, device="cpu", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    assert tr.vgg_precision == "f16grad" and ip.p2_precision() == "f16grad"
