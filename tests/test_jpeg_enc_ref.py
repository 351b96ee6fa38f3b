"""The encoder's restatement (tests/jpeg_enc_ref.py) against Pillow's bytes: the fixture (tests/golden/g24_jpeg_encode.npz, written
with Pillow 12.2.0) for every case, and a fresh ``Image.save`` where the installed Pillow is that version.  No GPU, no library.
Byte identity throughout: libjpeg's forward pipeline is integer arithmetic."""
import io

import numpy as np
import pytest

import jpeg_enc_ref as E
import jpeg_ref as R


@pytest.fixture(scope="module")
def cases():
    return E.load_fixture()


def test_the_case_list_is_whole(cases):
    names = [c[0] for c in E.case_list()]
    assert list(cases) == names and len(names) == len(E.SIZES) * 3 * 4 * 3 + 2
    for (h, w) in E.SIZES:
        for kind in E.CONTENTS:
            assert cases[f"{h}x{w}_{kind}_q75_s420"]["img"].shape == (h, w, 3)
    sat = cases["64x64_sat_q100_s444"]["img"]
    assert set(np.unique(sat)) == {0, 255}
    assert sum(c["img"].ndim == 2 for c in cases.values()) == 2


def test_restatement_coefficients_equal_the_fixtures(cases):
    """Image -> coefficients, every dummy block included, against what Pillow's stream holds."""
    for name, c in cases.items():
        coef, qtab, geo = E.image_coefficients(c["img"], c["quality"], c["subsampling"])
        assert np.array_equal(qtab, c["qtab"]), name
        got = E.flat_coef(coef)
        assert got.shape == c["coef"].shape and np.array_equal(got, c["coef"]), (name, int((got != c["coef"]).sum()))


def test_restatement_bytes_equal_the_fixtures(cases):
    for name, c in cases.items():
        got = E.encode(c["img"], c["quality"], c["subsampling"])
        assert got == c["data"], (name, len(got), len(c["data"]))


def test_entropy_coder_round_trips_through_the_decoders_restatement(cases):
    """The fixture's coefficients -> bytes -> tests/jpeg_ref.py's entropy decode -> the coefficients."""
    for name in ("17x23_noise_q95_s420", "8x24_sat_q100_s420", "gray_17x23_noise_q75", "37x45_ramp_q30_s422"):
        c = cases[name]
        geo = E.geometry(*c["img"].shape[:2], 1 if c["img"].ndim == 2 else 3, *E.SAMPLING[c["subsampling"]])
        data = E.entropy_encode(E.split_coef(c["coef"], geo), geo, c["qtab"])
        assert data == c["data"], name
        coef, qtab = R.entropy_decode(data)
        assert np.array_equal(R.flat_coef(coef), c["coef"]) and np.array_equal(qtab, c["qtab"]), name


def test_out_of_range_coefficients_are_refused(cases):
    c = cases["8x8_noise_q75_s444"]
    geo = E.geometry(8, 8, 3, 1, 1)
    coef = [a.copy() for a in E.split_coef(c["coef"], geo)]
    coef[0][0, 0, 5] = 1024
    with pytest.raises(E.OutOfRange):
        E.entropy_encode(coef, geo, c["qtab"])


def test_quant_tables_follow_libjpegs_scaling():
    assert np.array_equal(E.quant_tables(50)[0], E.BASE_LUMA) and np.array_equal(E.quant_tables(50)[1], E.BASE_CHROMA)
    assert (E.quant_tables(100) == 1).all() and E.quant_tables(1).max() == 255
    assert E.quant_tables(75)[0][:4].tolist() == [8, 6, 5, 8]


def test_restatement_equals_a_fresh_pillow_save(cases):
    PIL = pytest.importorskip("PIL")
    if PIL.__version__ != "12.2.0":
        pytest.skip(f"the bytes are pinned to Pillow 12.2.0, installed: {PIL.__version__}")
    from PIL import Image
    g = np.random.default_rng(99)
    sub = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
    for (h, w), q, s in (((19, 33), 60, "4:2:0"), ((40, 9), 88, "4:2:2"), ((10, 50), 5, "4:4:4"), ((34, 2), 100, "4:2:0")):
        img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=q, subsampling=sub[s])
        assert E.encode(img, q, s) == buf.getvalue(), (h, w, q, s)
    for name in list(cases)[::37]:
        c = cases[name]
        buf = io.BytesIO()
        if c["img"].ndim == 2:
            Image.fromarray(c["img"], "L").save(buf, "JPEG", quality=c["quality"])
        else:
            Image.fromarray(c["img"], "RGB").save(buf, "JPEG", quality=c["quality"], subsampling=sub[c["subsampling"]])
        assert buf.getvalue() == c["data"], name
