"""GPU: the host-side pieces every fused trainer of the seq kernels shares -- ``seq_train.TrainLayer`` (operand images, Adam's
moments, the update sweep's table entry) and ``seq._GraphCache.clear`` -- at the smallest shapes that take every branch."""
import pytest
import torch

from synth import seeded_randn

pytestmark = pytest.mark.gpu

# (name, out, in, pieces, kp): a single piece that needs padding both ways; the probe's first linear over two 24-wide embedders
PADDED = {"one-piece": (51, 100, None, None), "two-piece": (51, 48, [(0, 24, 0), (24, 24, 64)], 128)}


def _layer(tag):
    from behavior_driven_video_synthesis_amd.seq_train import TrainLayer
    m, k, pieces, kp = PADDED[tag]
    lin = torch.nn.Linear(k, m).cuda()
    lin.weight.data.copy_(seeded_randn(f"tl.{tag}.w", (m, k), 9))
    lin.bias.data.copy_(seeded_randn(f"tl.{tag}.b", (m,), 9))
    return lin, TrainLayer(tag, lin.weight, lin.bias, pieces, kp)


def _valid(lay):
    """The elements of the [64, 128] weight image / [64] bias image that belong to the parameter."""
    w = torch.zeros(64, 128, dtype=torch.bool, device="cuda")
    for _, n, dst in lay.pieces:
        w[:lay.rows, dst:dst + n] = True
    b = torch.zeros(64, dtype=torch.bool, device="cuda")
    b[:lay.rows] = True
    return w, b


def test_a_layer_that_fits_is_its_own_image():
    from behavior_driven_video_synthesis_amd.seq_train import TrainLayer
    lin = torch.nn.Linear(64, 64).cuda()
    w0, b0 = lin.weight.detach().clone(), lin.bias.detach().clone()
    lay = TrainLayer("fits", lin.weight, lin.bias)
    assert lay.w.data_ptr() == lin.weight.data_ptr() and lay.b.data_ptr() == lin.bias.data_ptr() and lay.inplace
    assert (lay.mp, lay.kp, lay.tiles()) == (64, 64, 1) and lay.m is None
    lay.load()
    lay.write_back()
    torch.cuda.synchronize()
    assert torch.equal(lin.weight, w0) and torch.equal(lin.bias, b0)


@pytest.mark.parametrize("tag", list(PADDED))
def test_a_padded_layer_round_trips_bit_for_bit_and_its_padding_stays_zero(tag):
    lin, lay = _layer(tag)
    w0, b0 = lin.weight.detach().clone(), lin.bias.detach().clone()
    assert not lay.w_inplace and not lay.b_inplace and tuple(lay.w.shape) == (64, 128) and tuple(lay.b.shape) == (64,)
    assert lay.tiles() == 2 and lay.m is None                     # the moments wait for the first fused step
    vw, vb = _valid(lay)
    assert int(vw.sum()) == w0.numel() and torch.equal(lay.w[vw].sort().values, w0.flatten().sort().values)
    # parameter -> image -> parameter
    lin.weight.data.zero_()
    lin.bias.data.zero_()
    lay.write_back()
    torch.cuda.synchronize()
    assert torch.equal(lin.weight, w0) and torch.equal(lin.bias, b0)
    lin.weight.data.mul_(2.0)
    lay.load()
    lay.write_back()
    torch.cuda.synchronize()
    assert torch.equal(lin.weight, 2.0 * w0) and torch.equal(lin.bias, b0)
    # moments: before the first step zeros in the parameters' shapes and nothing allocated
    (m, v), (bm, bv) = lay.moments()
    assert lay.m is None and m.shape == w0.shape and bm.shape == b0.shape and not any(t.any() for t in (m, v, bm, bv))
    want = [(seeded_randn(f"tl.{tag}.m", tuple(w0.shape), 9).cuda(), seeded_randn(f"tl.{tag}.v", tuple(w0.shape), 9).cuda() ** 2),
            (seeded_randn(f"tl.{tag}.bm", tuple(b0.shape), 9).cuda(), seeded_randn(f"tl.{tag}.bv", tuple(b0.shape), 9).cuda() ** 2)]
    lay.set_moments(*want)
    images = [t.clone() for t in (lay.m, lay.v, lay.bm, lay.bv)]
    got = lay.moments()
    for (a, b), (c, d) in zip(got, want):
        assert torch.equal(a, c) and torch.equal(b, d)
        assert a.data_ptr() not in [t.data_ptr() for t in (lay.m, lay.v, lay.bm, lay.bv)]      # copies
    lay.set_moments(*got)
    for now, before in zip((lay.m, lay.v, lay.bm, lay.bv), images):
        assert torch.equal(now, before)
    for img, valid in ((lay.w, vw), (lay.m, vw), (lay.v, vw), (lay.b, vb), (lay.bm, vb), (lay.bv, vb)):
        assert not img[~valid].any() and img[valid].any()
    lay.set_moments(None, None)                                    # a parameter without state: Adam starts from zero
    assert not any(t.any() for t in (lay.m, lay.v, lay.bm, lay.bv))


def test_the_sweep_entry_is_the_positional_one():
    """``TrainLayer.dw_entry`` names ``vunet_seq_dw_layer``'s fields; the values are those of the positional call it replaces."""
    from behavior_driven_video_synthesis_amd.seq_train import SeqDwLayer
    _, lay = _layer("one-piece")
    dz, x, raw = (torch.zeros(16, n, device="cuda") for n in (64, 192, 128))
    g, bg = torch.zeros_like(lay.w), torch.zeros_like(lay.b)
    # write mode (autograd): no moments are allocated for it
    got = lay.dw_entry(dz.data_ptr(), 64, x.data_ptr(), 192, 7, grads=(g, bg), kv=100, nchunk=2, dx_raw=raw.data_ptr())
    assert lay.m is None
    want = SeqDwLayer(lay.w.data_ptr(), None, None, g.data_ptr(), lay.b.data_ptr(), None, None, bg.data_ptr(), dz.data_ptr(),
                      x.data_ptr(), 64, 128, 64, 192, 7, 2, 100, 2, 0, 0, raw.data_ptr())
    for name, _ in SeqDwLayer._fields_:
        assert getattr(got, name) == getattr(want, name), name
    assert lay.tiles(2) == 2 and lay.tiles(4) == 2
    # the fused update: on the layer's moments, every column of the image valid unless told otherwise
    got = lay.dw_entry(dz.data_ptr(), 64, x.data_ptr(), 128, 0)
    want = SeqDwLayer(lay.w.data_ptr(), lay.m.data_ptr(), lay.v.data_ptr(), None, lay.b.data_ptr(), lay.bm.data_ptr(), lay.bv.data_ptr(),
                      None, dz.data_ptr(), x.data_ptr(), 64, 128, 64, 128, 0, 2, 128, 1, 0, 0, None)
    for name, _ in SeqDwLayer._fields_:
        assert getattr(got, name) == getattr(want, name), name
    assert bytes(got) == bytes(want)


def test_clear_forgets_the_recordings_and_the_warm_up():
    from behavior_driven_video_synthesis_amd.seq import _GraphCache
    from behavior_driven_video_synthesis_amd.seq_train import AdamState
    adam = AdamState("cuda", 1e-3)
    cache = _GraphCache()
    cache.enabled = True
    assert [cache.run_step("k", adam.tick) for _ in range(3)] == ["eager", "captured", "replayed"]
    assert list(cache.graphs) == ["k"]
    cache.clear()
    assert not cache.graphs and not cache._warmed
    assert cache.run_step("k", adam.tick) == "eager"
    assert adam.step == 4                                          # every call ran the step exactly once
