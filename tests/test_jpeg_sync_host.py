"""The host side of the device entropy decoder -- ``vunet_jpeg_scan_segments`` and ``vunet_jpeg_huffdec_rows`` of
csrc/jpeg_entropy.h, pure host functions -- against the restatement (tests/jpeg_sync_ref.py) on tests/golden/g23_jpeg.npz, and
tools/jpeg_sync_check.cpp, which runs the kernels' own walk (csrc/jpeg_sync.h) on the CPU under the sanitizers.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ref as R
import jpeg_sync_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = R.load_fixture()


@pytest.fixture(scope="module")
def J():
    from behavior_driven_video_synthesis_amd import jpeg_decode
    return jpeg_decode


def _scan(J, data):
    from behavior_driven_video_synthesis_amd import _lib
    return J._scan(_lib.lib(), data, J._parse_c(data))


def test_the_header_constants_are_what_python_and_the_restatement_read(J):
    assert J.SUBSEQ_BYTES == SR.SUBSEQ_BYTES and J.SUBSEQ_BYTES % 8 == 0 and J.GROUP % 64 == 0
    assert ctypes.sizeof(J.Subseq) == 40 and J.TAB_BYTES == 4 * (1024 + 72 + 68 + 256) + 40


def test_scan_segments_equals_the_restatement_on_g23(J):
    for name, c in FIX["cases"].items():
        hdr = R.parse(c["data"])
        rc, segs, tabs = _scan(J, c["data"])
        assert rc == 0 and [tuple(s) for s in segs.tolist()] == SR.segments(c["data"], hdr), name
        assert np.array_equal(tabs[:2 * 64 * hdr["ncomp"]].view(np.uint16), c["qtab"].reshape(-1)), name
        tail = tabs[384:][-40:].view(np.int32)                 # dc[3], ac[3], blocks per MCU, luma blocks, restart interval
        per_mcu = hdr["hsamp"] * hdr["vsamp"] + 2 if hdr["ncomp"] == 3 else 1
        assert tail[6:9].tolist() == [per_mcu, max(per_mcu - 2, 1), hdr["restart"]], name
        assert set(tail[:hdr["ncomp"]].tolist()) <= {0, 1} and set(tail[3:3 + hdr["ncomp"]].tolist()) <= {2, 3}
        # the flattened look-up resolves every code of at most nine bits to (length, symbol), component by component
        for comp in range(hdr["ncomp"]):
            for kind, slot in ((0, tail[comp]), (1, tail[3 + comp])):
                look = tabs[384 + 1420 * slot:384 + 1420 * slot + 1024].view(np.uint16)
                for (length, code), sym in R._codebook(hdr["dc" if kind == 0 else "ac"][comp]).items():
                    if length <= 9:
                        assert look[code << (9 - length)] == (length << 8 | sym), (name, comp, kind, length, code)


def test_truncated_and_damaged_streams_come_out_irregular_or_refused(J):
    name, offsets = FIX["truncated"]
    whole = FIX["cases"][name]["data"]
    scan = R.parse(whole)["scan"]
    for off in offsets:
        data = whole[:off]
        try:
            info = J._parse_c(data)
        except J.JpegError:
            assert off < scan                                  # (the header itself is cut: never reaches the marker scan)
            continue
        from behavior_driven_video_synthesis_amd import _lib
        rc, segs, _ = J._scan(_lib.lib(), data, info)
        assert rc == J.IRREGULAR and len(segs) == 0, off       # no EOI in any prefix
        assert SR.segments(data, R.parse(data)) is None
    c = FIX["cases"]["s444_40x56_rst4_noise"]["data"]
    at = c.index(b"\xff\xd2")
    for bad in (c[:at + 1] + b"\xd3" + c[at + 2:], c[:at] + b"\xff" + c[at:], c[:at] + c[at + 2:], c[:at] + b"\xff\xd2" + c[at:]):
        assert _scan(J, bad)[0] == J.IRREGULAR
    # an info that is not the stream's, and a segment array that is too short
    from behavior_driven_video_synthesis_amd import _lib
    other = J._parse_c(whole)
    segs, n, tabs = np.zeros((9, 3), dtype=np.int64), ctypes.c_int64(0), np.zeros(384 + J.TAB_BYTES, dtype=np.uint8)
    fn = _lib.lib().vunet_jpeg_scan_segments
    assert fn(c, len(c), ctypes.byref(other), segs.ctypes.data, 9, ctypes.byref(n), tabs.ctypes.data, tabs.ctypes.data + 384) == -1
    assert fn(c, len(c), ctypes.byref(J._parse_c(c)), segs.ctypes.data, 8, ctypes.byref(n), tabs.ctypes.data, tabs.ctypes.data + 384) == -1
    assert fn(c, len(c), ctypes.byref(J._parse_c(c)), segs.ctypes.data, 9, ctypes.byref(n), tabs.ctypes.data, tabs.ctypes.data + 384) == 0


def test_a_stream_with_three_dc_tables_is_irregular_and_still_brings_a_valid_table_row(J):
    """Baseline, and the host walk decodes it; the device has two DC and two AC slots, so the marker scan hands it to the host walk.
    Its table row goes up with the batch's and is checked with them: the MCU's shape and every table index must be valid."""
    from behavior_driven_video_synthesis_amd import _lib
    for name in ("s420_17x23_smooth", "s444_40x56_rst4_noise", "s422_33x41_noise"):
        c = FIX["cases"][name]
        data = SR.three_tables(c["data"])
        info = J._parse_c(data)
        coef, qtab = np.empty(info.ncoef, dtype=np.int16), np.empty(192, dtype=np.uint16)
        assert _lib.lib().vunet_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, qtab.ctypes.data) == 0
        assert np.array_equal(coef, c["coef"]), name
        rc, segs, tabs = J._scan(_lib.lib(), data, info)
        assert rc == J.IRREGULAR and len(segs) == 0, name
        assert np.array_equal(tabs[:384].view(np.uint16), c["qtab"].reshape(-1)), name
        tail = tabs[384:][-40:].view(np.int32)
        hv = info.hsamp * info.vsamp
        assert tail[6:9].tolist() == [hv + 2, hv, info.restart] and all(0 <= v <= 3 for v in tail[:6].tolist()), (name, tail.tolist())


def test_subsequence_rows_equal_the_restatements(J):
    from behavior_driven_video_synthesis_amd import _lib
    lib = _lib.lib()
    for name, c in FIX["cases"].items():
        data = c["data"]
        info = J._parse_c(data)
        rc, segs, _ = J._scan(lib, data, info)
        want = SR.subsequences(SR.segments(data, R.parse(data)), J.SUBSEQ_BYTES)
        cap = -(-len(want) // J.GROUP) * J.GROUP
        rows, made = (J.Subseq * cap)(), ctypes.c_int64(0)
        shift = 1000 - int(segs[0, 0])                         # the scan lies at byte 1000 of the batch's buffer
        assert lib.vunet_jpeg_huffdec_rows(segs.ctypes.data, len(segs), ctypes.byref(info), 3, shift, 2 * J.GROUP, rows, cap,
                                           ctypes.byref(made)) == 0 and made.value == cap, name
        assert lib.vunet_jpeg_huffdec_rows(segs.ctypes.data, len(segs), ctypes.byref(info), 3, shift, 2 * J.GROUP, rows, cap - 1,
                                           ctypes.byref(made)) == -1
        assert lib.vunet_jpeg_huffdec_rows(segs.ctypes.data, len(segs), ctypes.byref(info), 3, shift, 5, rows, cap, ctypes.byref(made)) == -1
        per_mcu = info.hsamp * info.vsamp + 2 if info.ncomp == 3 else 1
        for i, w in enumerate(want):
            r, (b, e, mcu0) = rows[i], segs[w["seg"]].tolist()
            assert (r.img, r.begin, r.end, r.seg_begin, r.seg_end) == (3, w["begin"] + shift, w["end"] + shift, b + shift, e + shift), (name, i)
            assert r.flags == (1 if w["first"] else 0) | (2 if w["last"] else 0) | (4 if w["seg"] + 1 == len(segs) else 0), (name, i)
            assert r.first_block == mcu0 * per_mcu and rows[r.seg_row - 2 * J.GROUP].flags & 1 and r.seg_row <= 2 * J.GROUP + i
        assert sum(rows[i].seg_blocks for i in range(len(want)) if rows[i].flags & 1) == info.nblocks, name
        assert all(rows[i].flags == 8 and rows[i].img == 3 for i in range(len(want), cap)), name


def test_the_kernels_walk_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/jpeg_sync_check.cpp (its own ``main``; neither HIP nor the library is involved) built with -fsanitize=address,undefined:
    whole streams, every prefix and seeded bit flips at subsequences of 8, 16 and VUNET_JPEG_SUBSEQ_BYTES bytes."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_sync_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "jpeg_sync_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower() or "sanitize" in build.stderr.lower()):
        pytest.skip("this compiler has no address / undefined-behaviour sanitizers")
    assert build.returncode == 0, build.stderr
    names = list(FIX["cases"])                                 # all of g23, in four processes side by side (each input is independent)
    paths = []
    for n in names:
        paths.append(str(tmp_path / (n + ".jpg")))
        with open(paths[-1], "wb") as f:
            f.write(FIX["cases"][n]["data"])
    order = sorted(paths, key=os.path.getsize, reverse=True)   # (the cost grows with the square of a stream's size)
    shares = [order[i::4] for i in range(4)]
    procs = [subprocess.Popen([exe] + share, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for share in shares]
    for share, proc in zip(shares, procs):
        out, _ = proc.communicate()
        assert proc.returncode == 0, out
        assert f"from {len(share)} streams" in out and "decoded, equal to the host decoder" in out and "FAILURES" not in out
