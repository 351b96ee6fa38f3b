"""The host layer the JPEG codec modules share (behavior_driven_video_synthesis_amd/jpeg_host.py), without a GPU: the one writer of
the descriptor table, the grow-only arena and the byte layouts of the three uploads, these against the offset formulas the two
modules spelled out by hand before the helper existed (copied here as literals: the C entry points check 16-byte alignment and the
bounds tests build their bad arguments from these offsets, so none of them may move)."""
import ctypes

import pytest
import torch

from behavior_driven_video_synthesis_amd import _lib, jpeg_decode as D, jpeg_encode as E, jpeg_host as H


@pytest.fixture(scope="module")
def infos():
    """16 x 16 at 4:2:0, 17 x 23 at 4:4:4, gray 8 x 8."""
    out = []
    for h, w, ncomp, hs, vs in ((16, 16, 3, 2, 2), (17, 23, 3, 1, 1), (8, 8, 1, 1, 1)):
        info = H.JpegInfoC()
        assert _lib.lib().vunet_jpeg_encode_info(h, w, ncomp, hs, vs, ctypes.byref(info)) == 0
        out.append(info)
    return out


def test_fill_rows_writes_every_field_and_the_running_sums(infos):
    rows, q_offs, slots = (H.JpegImg * 3)(), [0, 192, 0], [2, 0, 1]
    assert sorted(f for f, _ in H.JpegImg._fields_) == sorted(
        "coef_off plane_off q_off block0 slot height width ncomp hsamp vsamp bw0 bh0 bw1 bh1".split())
    totals = H.fill_rows(rows, infos, q_offs, slots)
    coef_at = block_at = 0
    for r, inf, q_off, slot in zip(rows, infos, q_offs, slots):
        assert (r.coef_off, r.plane_off, r.q_off, r.block0, r.slot) == (coef_at, coef_at, q_off, block_at, slot)
        assert (r.height, r.width, r.ncomp, r.hsamp, r.vsamp) == (inf.height, inf.width, inf.ncomp, inf.hsamp, inf.vsamp)
        assert (r.bw0, r.bh0, r.bw1, r.bh1) == (inf.bw0, inf.bh0, inf.bw1, inf.bh1)
        coef_at, block_at = coef_at + inf.ncoef, block_at + inf.nblocks
    assert totals == (coef_at, block_at) == (sum(i.ncoef for i in infos), sum(i.nblocks for i in infos))
    assert [i.nblocks for i in infos] == [6, 27, 1] and [i.ncoef for i in infos] == [384, 1728, 64]


def test_arena_keeps_what_is_large_enough_and_replaces_one_name_at_a_time():
    a = H.Arena(torch.device("cpu"), "planes coef scratch")
    assert a.stage is None and a.dev is None and a.scratch is None and a.entropy is None      # nothing is made until asked for
    planes, coef = a.get("planes", 100, torch.uint8), a.get("coef", 50, torch.int16, "pinned")
    assert planes.numel() == 100 and planes.dtype == torch.uint8 and coef.dtype == torch.int16 and a.planes is planes and a.coef is coef
    assert a.get("planes", 100, torch.uint8) is planes and a.get("planes", 7, torch.uint8) is planes
    larger = a.get("planes", 101, torch.uint8)
    assert larger is not planes and larger.numel() == 101 and a.planes is larger and a.coef is coef
    a.staging(64)
    stage, dev = a.stage, a.dev
    assert stage.numel() == dev.numel() == 64 and stage.dtype == dev.dtype == torch.uint8
    a.staging(64)
    assert a.stage is stage and a.dev is dev
    a.staging(65)
    assert a.stage is not stage and a.dev is not dev and a.planes is larger
    assert not any(t.is_pinned() for t in (a.stage, a.dev, a.planes, a.coef, a.get("scratch", 4, torch.int16, "pinned")))
    assert a.scratch.numel() == 4 and a.event is None


def _round(v, m):
    return (v + m - 1) // m * m


def _r4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("n", [1, 3, 16])
def test_the_decode_uploads_lie_where_they_lay(infos, n):
    coef_count = sum(infos[j % 3].ncoef for j in range(n))
    # the host route: descriptors | tables | coefficients
    q_off = n * ctypes.sizeof(H.JpegImg)
    c_off = _round(q_off + n * 384, 128)
    nbytes = c_off + 2 * coef_count
    assert D._host_plan(n, coef_count) == (n, nbytes, q_off, c_off, coef_count, max(coef_count, 16)) and c_off % 128 == 0
    # the device route: descriptors | tables | table rows | spans | subsequence rows | scan bytes
    for nsub, nscan in ((0, 0), (D.GROUP, 16), (3 * D.GROUP, 1000 * n + 48), (D.GROUP * n, 16 * 4097)):
        m = n
        q_off = m * ctypes.sizeof(D.JpegImg)
        t_off = _round(q_off + m * 384, 16)
        s_off = t_off + m * D.TAB_BYTES
        r_off = _round(s_off + 8 * m, 16)
        b_off = r_off + nsub * ctypes.sizeof(D.Subseq)
        nbytes = _round(b_off + nscan, 16) + 16
        offs, total = D._device_layout(m, nsub, nscan)
        assert (offs["imgs"], offs["qtab"], offs["tabs"], offs["spans"], offs["rows"], offs["bytes"], total) == \
            (0, q_off, t_off, s_off, r_off, b_off, nbytes)
        assert t_off % 16 == 0 and r_off % 16 == 0 and total % 16 == 0


@pytest.mark.parametrize("n,rows", [(1, 1), (3, 1), (3, 3), (5, 5)])
def test_the_encode_entropy_block_lies_where_it_lay(n, rows):
    spans_off = (4 * n + 15) // 16 * 16
    codes_off = spans_off + 16 * n
    want = (spans_off, codes_off, codes_off + 4096 * rows), (_r4(n), _r4(n) + _r4(2 * n), _r4(n) + _r4(2 * n) + n + 1)
    assert E._entropy_layout(n, rows) == want


def test_layout_places_each_piece_at_its_alignment():
    offs, total = H.layout(("a", 3, 1), ("b", 5, 16), ("c", 0, 4), ("d", 1, 128))
    assert offs == {"a": 0, "b": 16, "c": 24, "d": 128} and total == 129
    assert H.layout() == ({}, 0)
