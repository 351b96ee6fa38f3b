"""The restatement of the device entropy decoder's rounds (tests/jpeg_sync_ref.py) against the decoder's restatement
(tests/jpeg_ref.py) and the fixture's coefficients (tests/golden/g23_jpeg.npz); the stream that never synchronises; and, at import,
what the GPU tests' streams make the walk meet at the header's subsequence size.  No GPU."""
import functools

import numpy as np
import pytest

import jpeg_ref as R
import jpeg_sync_ref as SR

FIX = R.load_fixture()
SIZES = sorted({8, 16, SR.SUBSEQ_BYTES})

# g23 and the stuffed stream are inputs of tests/test_hip_jpeg_huff_dec.py (tests 1, 5, 6, 7, 9): at VUNET_JPEG_SUBSEQ_BYTES they hold a
# stuffed 00 that is the first byte of a subsequence, an FF that is the last byte of one, a block that straddles three subsequences
# and a segment shorter than one subsequence.  A changed constant that loses one of them is reported here, not silently uncovered.
COVERAGE = SR.coverage([c["data"] for c in FIX["cases"].values()] + [SR.stuffed_stream()])
assert all(v > 0 for v in COVERAGE.values()), (SR.SUBSEQ_BYTES, COVERAGE)


@functools.lru_cache(maxsize=None)
def _oracle():
    """``jpeg_ref.entropy_decode`` of every stream of g23, in the library's layout; computed once and shared."""
    return {name: R.flat_coef(R.entropy_decode(c["data"])[0]) for name, c in FIX["cases"].items()}


@pytest.mark.parametrize("sub", SIZES)
def test_the_rounds_give_the_decoders_coefficients_on_all_of_g23(sub):
    rounds = {}
    for name, c in FIX["cases"].items():
        dec = SR.Decoder(c["data"], sub)
        got = dec.decode()
        assert got is not None, name
        assert np.array_equal(got, _oracle()[name]), name
        assert np.array_equal(got, c["coef"]), name            # (and so the fixture's, which are the library's)
        longest = max(sum(1 for r in dec.rows if r["seg"] == s) for s in range(len(dec.segs)))
        assert dec.rounds <= longest + 1, (name, dec.rounds, longest)
        rounds[name] = dec.rounds
    if sub == 8:
        assert max(rounds.values()) > 3                        # (small subsequences do need rounds: the bound is not idle)


def test_segments_of_restart_streams_and_irregular_layouts():
    c = FIX["cases"]["s444_40x56_rst4_noise"]["data"]
    hdr = R.parse(c)
    segs = SR.segments(c, hdr)
    assert hdr["restart"] == 4 and len(segs) == 9 and [s[2] for s in segs] == list(range(0, 36, 4))
    assert all(c[e:e + 2] == bytes([0xFF, 0xD0 + (i & 7)]) for i, (_, e, _) in enumerate(segs[:-1])) and c[segs[-1][1]:] == b"\xff\xd9"
    assert len(SR.segments(FIX["cases"]["s420_17x23_smooth"]["data"], R.parse(FIX["cases"]["s420_17x23_smooth"]["data"]))) == 1
    at = c.index(b"\xff\xd2")
    for bad in (c[:at + 1] + b"\xd3" + c[at + 2:],              # a restart marker out of sequence
                c[:at] + b"\xff" + c[at:],                     # a fill byte
                c[:-2], c[:-1],                                # no EOI; an FF at the end of the data
                c[:at] + c[at + 2:],                           # one marker, and so one segment, too few
                c[:at] + b"\xff\xd2" + c[at:]):                # an empty segment
        assert SR.segments(bad, hdr) is None
        assert SR.Decoder(bad).decode() is None


def test_a_stream_with_three_dc_tables_is_the_same_image_to_the_restatement():
    """``three_tables`` changes table ids only: the restatement, which knows no table slots, decodes it to the same coefficients."""
    name = "s420_17x23_smooth"
    data = SR.three_tables(FIX["cases"][name]["data"])
    assert data != FIX["cases"][name]["data"] and R.parse(data)["dc"][2] == R.parse(data)["dc"][1]
    assert np.array_equal(R.flat_coef(R.entropy_decode(data)[0]), _oracle()[name])
    assert np.array_equal(SR.Decoder(data).decode(), _oracle()[name])


def test_the_constant_colour_stream_never_synchronises():
    """The constant (200, 30, 90) frame of the GPU test, built as it builds it (quality 75, 4:2:0; the host coder's bytes are
    encode_batch's): a guessed state never falls into step, so the true states advance one subsequence per round -- as many rounds as
    subsequences (and one more that finds nothing changed).  This is the worst case the bound of the host loop exists for."""
    dec = SR.Decoder(SR.never_stream())
    dec.synchronise()
    n = len(dec.rows)
    assert n > 256 and len(dec.segs) == 1                      # more than one workgroup of subsequences
    assert dec.rounds - 1 == n, (dec.rounds, n, SR.SUBSEQ_BYTES)
    assert dec.walks[0] == n and dec.walks[-2:] == [1, 0] and dec.walks[n // 2] <= 2
    # ... while in a noise frame guessed states do fall into step, and the work per round shrinks fast
    noise = SR.Decoder(FIX["cases"]["s420_50x70_q100_noise"]["data"])
    assert noise.decode() is not None and noise.rounds < len(noise.rows) and noise.walks[5] < noise.walks[0] // 2
