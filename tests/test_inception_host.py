"""CPU-only checks of the Inception-v3 host side (models/inception.py): torchvision's state-dict layout, the layer plan's
geometry and concat offsets, the float64 batch-norm fold, the packing, and that the path is inference only and GPU only."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

from behavior_driven_video_synthesis_amd.models import inception as I
from behavior_driven_video_synthesis_amd.models.imagenet_pretrained import FIDInceptionModel, InceptionV3

import inception_ref as R


def expected_keys():
    """The 566 names, built from the naming rule of the issue (not from the package's table): 94 BasicConv2d x 6 + fc."""
    convs = ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "Conv2d_3b_1x1", "Conv2d_4a_3x3"]
    a = ["branch1x1", "branch5x5_1", "branch5x5_2", "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3", "branch_pool"]
    b = ["branch3x3", "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"]
    c = ["branch1x1", "branch7x7_1", "branch7x7_2", "branch7x7_3"] + ["branch7x7dbl_%d" % i for i in range(1, 6)] + ["branch_pool"]
    d = ["branch3x3_1", "branch3x3_2"] + ["branch7x7x3_%d" % i for i in range(1, 5)]
    e = ["branch1x1", "branch3x3_1", "branch3x3_2a", "branch3x3_2b", "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3a",
         "branch3x3dbl_3b", "branch_pool"]
    for blk, names in (("Mixed_5b", a), ("Mixed_5c", a), ("Mixed_5d", a), ("Mixed_6a", b), ("Mixed_6b", c), ("Mixed_6c", c),
                       ("Mixed_6d", c), ("Mixed_6e", c), ("Mixed_7a", d), ("Mixed_7b", e), ("Mixed_7c", e)):
        convs += [f"{blk}.{n}" for n in names]
    assert len(convs) == 94
    keys = [f"{cv}.{s}" for cv in convs for s in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var",
                                                  "bn.num_batches_tracked")]
    return convs, keys + ["fc.weight", "fc.bias"]


@pytest.fixture(scope="module")
def net():
    return InceptionV3()


def test_state_dict_has_exactly_torchvisions_566_keys(net):
    convs, keys = expected_keys()
    sd = net.state_dict()
    assert len(keys) == 566 and list(sd.keys()) == keys
    assert list(FIDInceptionModel().state_dict().keys()) == keys
    assert list(I.SPECS) == convs
    for name, (cin, cout, k, s, p) in I.SPECS.items():
        assert tuple(sd[name + ".conv.weight"].shape) == (cout, cin) + k
        assert net.layer(name).bn.eps == 1e-3


def test_parameter_counts(net):
    body = sum(p.numel() for n, p in net.named_parameters() if not n.startswith("fc."))
    assert body == 21785568
    assert sum(p.numel() for p in net.parameters()) == 23834568
    assert not any(p.requires_grad for p in net.parameters())


def test_a_state_dict_with_auxlogits_loads(net):
    sd = {k: v.clone() for k, v in InceptionV3(seed=7).state_dict().items()}
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    sd["AuxLogits.fc.bias"] = torch.zeros(1000)
    m = InceptionV3(state_dict=sd)
    assert torch.equal(m.fc.weight, sd["fc.weight"]) and torch.equal(m.Mixed_6c.branch7x7_2.conv.weight, sd["Mixed_6c.branch7x7_2.conv.weight"])
    FIDInceptionModel(state_dict=sd)
    with pytest.raises(RuntimeError):
        InceptionV3(state_dict={k: v for k, v in sd.items() if k != "fc.bias"})


def test_plan_map_sizes_and_concat_offsets(net):
    plan = net.plan(2, 299, 299)
    widths = [w for _, w in plan.map_sizes]
    stem, blocks = widths[:7], widths[7:]
    dedup = [w for i, w in enumerate(blocks) if i == 0 or blocks[i - 1] != w]
    assert stem + dedup == [149, 147, 147, 73, 73, 71, 35, 35, 17, 8]
    assert all(h == w for h, w in plan.map_sizes)
    assert [plan.block_out[b[0]][0] for b in I.BLOCKS] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    assert plan.block_slices["Mixed_5b"] == [(0, 64), (64, 64), (128, 96), (224, 32)]
    assert plan.block_slices["Mixed_5d"] == [(0, 64), (64, 64), (128, 96), (224, 64)]
    assert plan.block_slices["Mixed_6a"] == [(0, 384), (384, 96), (480, 288)]
    assert plan.block_slices["Mixed_6c"] == [(0, 192), (192, 192), (384, 192), (576, 192)]
    assert plan.block_slices["Mixed_7a"] == [(0, 320), (320, 192), (512, 768)]
    assert plan.block_slices["Mixed_7c"] == [(0, 320), (320, 384), (704, 384), (1088, 384), (1472, 384), (1856, 192)]
    for name, slices in plan.block_slices.items():   # the slices tile the block's output
        off = 0
        for o, c in slices:
            assert o == off
            off += c
        assert off == plan.block_out[name][0]
    # 94 convolutions + fc, 3 + 4 + 2 average pools, 2 stem pools, 2 max-pool branches, the global average
    fns = [s.fn for s in plan.steps]
    assert fns.count("conv") == 95 and fns.count("pool") == 13 and fns.count("gap") == 1 and fns.count("input") == 0
    assert net.plan(3, 75, 75).map_sizes[-1] == (1, 1)
    assert net.plan(3, 107, 91).map_sizes[0] == (53, 45)
    with pytest.raises(ValueError):
        net.plan(1, 74, 299)
    fid = FIDInceptionModel().plan(2, 128, 96, "fid")
    assert fid.steps[0].fn == "input" and fid.steps[0].args == (2, 128, 96, 2) and fid.map_sizes[0] == (149, 149)
    assert [s.desc.mode for s in fid.steps if s.label.startswith("stem_pool")] == [1, 1]
    assert [s.desc.mode for s in plan.steps if s.label.startswith("stem_pool")] == [0, 0]


def test_plan_buffers_lie_inside_the_arena_and_live_ones_do_not_overlap(net):
    """Every launch reads and writes inside the arena, and no launch of a block writes into a buffer another launch of the same
    block still reads (scratch is shared between blocks only)."""
    plan = net.plan(2, 107, 91)
    n = plan.n
    for s in plan.steps:
        if s.fn == "conv":
            d = s.desc
            src, dst = n * d.x_ctot * d.H * d.W, n * d.y_ctot * d.Ho * d.Wo
        elif s.fn == "pool":
            d = s.desc
            src, dst = n * d.x_ctot * d.H * d.W, n * d.y_ctot * d.Ho * d.Wo
        else:
            src, dst = s.args[0] * s.args[1], s.args[0]
        assert 0 <= s.dst and s.dst + dst <= plan.arena_floats
        if s.src is not None:
            assert 0 <= s.src and s.src + src <= plan.arena_floats
            assert s.src + src <= s.dst or s.dst + dst <= s.src, s.label
    by_block = {}
    for s in plan.steps:
        by_block.setdefault(s.label.split(".")[0] if s.label.startswith("Mixed") else "stem", []).append(s)
    for name, steps in by_block.items():
        spans = {}
        for s in steps:
            spans[s.dst] = n * s.desc.y_ctot * s.desc.Ho * s.desc.Wo if s.desc is not None else s.args[0]
        offs = sorted(spans)
        for a, b in zip(offs, offs[1:]):
            assert a + spans[a] <= b, name


def test_bn_fold_in_float64_matches_batch_norm_after_conv():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(10, 6, 1, 7, generator=g)
    gamma, beta = torch.rand(10, generator=g) + 0.5, torch.randn(10, generator=g)
    mean, var = torch.randn(10, generator=g), torch.rand(10, generator=g) * 3 + 0.01
    x = torch.randn(2, 6, 9, 11, generator=g, dtype=torch.float64)
    wf, bf = I.fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    ref = F.batch_norm(F.conv2d(x, w.double(), None, padding=(0, 3)), mean.double(), var.double(), gamma.double(), beta.double(),
                       training=False, eps=1e-3)
    got = F.conv2d(x, wf, bf, padding=(0, 3))
    assert float((got - ref).abs().max()) < 1e-12
    # torchvision's transform_input in front of the unpadded first convolution, folded
    x3 = torch.randn(2, 3, 9, 11, generator=g, dtype=torch.float64)
    w3, b3 = torch.randn(5, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
    wt, bt = I.fold_input_affine(w3, b3, [s / 0.5 for s in I.STD], [(m - 0.5) / 0.5 for m in I.MEAN])
    assert float((F.conv2d(x3, wt, bt, stride=2) - F.conv2d(R.transform_input(x3), w3, b3, stride=2)).abs().max()) < 1e-12


def test_packing_is_k_major_and_zero_padded():
    w = torch.arange(5 * 3 * 1 * 7, dtype=torch.float64).view(5, 3, 1, 7)
    p = I.pack_weight(w)
    assert p.dtype == torch.float32 and tuple(p.shape) == (64, 64)
    assert torch.equal(p[:21, :5], w.view(5, 21).t().float())
    assert float(p[21:].abs().sum()) == 0.0 and float(p[:, 5:].abs().sum()) == 0.0


def test_the_path_is_inference_only_and_gpu_only(net):
    with pytest.raises(RuntimeError):
        net.train()
    with pytest.raises(RuntimeError):
        FIDInceptionModel().train(True)
    assert net.eval() is net and not net.training
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 75, 75))
    with pytest.raises(ValueError):
        InceptionV3(stem_pool="min")


def test_ctypes_structs_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vunet_inception.h")).read(), flags=re.S)
    for cname, cls in (("vunet_convg_desc", I.ConvgDesc), ("vunet_pool2d_desc", I.Pool2dDesc)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname, txt, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                typ, names = decl.split(None, 1)
                assert typ == "int32_t"
                fields += [n.strip() for n in names.split(",")]
        assert [f[0] for f in cls._fields_] == fields, cname
        assert all(f[1] is ctypes.c_int32 for f in cls._fields_)
    assert int(re.search(r"#define VUNET_CONVG_KC (\d+)", txt).group(1)) == I.KC
    assert int(re.search(r"#define VUNET_CONVG_MT (\d+)", txt).group(1)) == I.MT
    assert int(re.search(r"#define VUNET_INCEPTION_SIZE (\d+)", txt).group(1)) == I.SIZE
    from behavior_driven_video_synthesis_amd import _lib
    protos = _lib.declared_prototypes()
    assert len(protos["vunet_convg"]) == 6 and len(protos["vunet_pool2d"]) == 4 and len(protos["vunet_global_avgpool"]) == 5
    assert protos["vunet_global_avgpool"][2] is ctypes.c_int64 and len(protos["vunet_inception_input"]) == 7


def test_the_restatement_agrees_with_itself_across_dtypes_and_stem_pools(net):
    """The float64 restatement and its fp32 run agree to fp32 noise on the smallest input, and the two stem pools differ."""
    sd = net.state_dict()
    x = torch.randn(1, 3, 75, 75, generator=torch.Generator().manual_seed(0))
    f64 = R.features(R.cast(sd, torch.float64), x.double())
    f32 = R.features(R.cast(sd, torch.float32), x)
    assert tuple(f64.shape) == (1, 2048) and float(f64.abs().max()) > 1e-2
    assert float((f32.double() - f64).abs().max()) < 1e-4 * float(f64.abs().max())
    favg = R.features(R.cast(sd, torch.float64), x.double(), stem_pool="avg")
    assert float((favg - f64).abs().max()) > 1e-2 * float(f64.abs().max())
