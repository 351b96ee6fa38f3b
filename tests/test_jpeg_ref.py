"""The restatement of the baseline JPEG decoder (tests/jpeg_ref.py) against Pillow's bytes -- through the fixture
(tests/golden/g23_jpeg.npz, written with Pillow 12.2.0 / libjpeg-turbo) and, where PIL imports, directly on seeded random cases.
Zero differing bytes: there is no tolerance.  No GPU."""
import io

import numpy as np
import pytest

import jpeg_ref as R


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


def test_fixture_holds_the_cases_the_decoder_is_held_to(fixture):
    cases = fixture["cases"]
    assert len(cases) == 20 and len({n.rsplit("_", 1)[0] for n in cases}) == 10
    hdrs = {n: R.parse(c["data"]) for n, c in cases.items()}
    assert {(h["ncomp"], h["hsamp"], h["vsamp"]) for h in hdrs.values()} == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)}
    assert sum(1 for h in hdrs.values() if h["restart"]) == 4
    assert max(max(c["rgb"].shape[:2]) for c in cases.values()) <= 70
    assert sorted(fixture["refused"]) == ["cmyk", "progressive"]
    name, offs = fixture["truncated"]
    scan = hdrs[name]["scan"]
    assert hdrs[name]["hsamp"] == hdrs[name]["vsamp"] == 2
    assert min(offs) < 20 and any(o > scan for o in offs) and len(cases[name]["data"]) - 2 in offs and len(offs) >= 12


def test_restatement_reproduces_every_fixture_image(fixture):
    for name, c in fixture["cases"].items():
        got = R.decode(c["data"])
        assert got.shape == c["rgb"].shape and np.array_equal(got, c["rgb"]), (name, int((got != c["rgb"]).sum()))
        coef, qtab = R.entropy_decode(c["data"])
        assert np.array_equal(R.flat_coef(coef), c["coef"]) and np.array_equal(qtab, c["qtab"]), name


def test_checkerboard_clamps_on_both_sides(fixture):
    """The hard 0 / 255 checkerboard overshoots: the unclamped IDCT output leaves [0, 255] on both sides."""
    c = fixture["cases"]["checker_24x24_smooth"]
    coef, qtab = R.entropy_decode(c["data"])
    v = (coef[0].astype(np.int64) * qtab[0].astype(np.int64)).reshape(coef[0].shape[:-1] + (8, 8))
    ws = np.swapaxes(R._idct_1d(np.swapaxes(v, -1, -2), 13, 11), -1, -2)
    raw = R._idct_1d(ws, 13, 18) + 128
    assert raw.min() < 0 and raw.max() > 255


def test_refused_and_truncated_streams_raise(fixture):
    for name, data in fixture["refused"].items():
        with pytest.raises(R.Unsupported):
            R.parse(data)
    name, offs = fixture["truncated"]
    data = fixture["cases"][name]["data"]
    for o in offs:
        if o >= len(data) - 2:          # only the EOI is gone: the scan itself is whole
            continue
        with pytest.raises(R.Corrupt):
            R.decode(data[:o])


def _random_cases(n=40, seed=23):
    g = np.random.default_rng(seed)
    for i in range(n):
        h, w = int(g.integers(1, 65)), int(g.integers(1, 65))
        kind = int(g.integers(0, 4))                    # 0..2: Pillow's subsampling code (4:4:4, 4:2:2, 4:2:0); 3: grayscale
        if g.integers(0, 2):
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.stack([(np.sin(xx / 5.0 + k) + np.cos(yy / 7.0 - k)) * 60 + 128 for k in range(3)], axis=2)
            img = np.clip(img + g.normal(0, 3, img.shape), 0, 255).astype(np.uint8)
        else:
            img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        kw = dict(quality=int(g.integers(20, 101)), optimize=bool(g.integers(0, 2)))
        r = int(g.integers(0, 3))
        if r == 1:
            kw["restart_marker_blocks"] = int(g.integers(1, 6))
        elif r == 2:
            kw["restart_marker_rows"] = 1
        if i < 4:                                       # down-sampled widths 1 and 2 (plain replication) and 3 (fancy), always
            w, kind = (1, 2, 4, 5)[i], 1 + i % 2
            img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        yield i, img, kind, kw


def test_restatement_reproduces_pillow_on_random_cases():
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for i, img, kind, kw in _random_cases():
        im = Image.fromarray(img, "RGB")
        buf = io.BytesIO()
        if kind == 3:
            im.convert("L").save(buf, "JPEG", **kw)
        else:
            im.save(buf, "JPEG", subsampling=kind, **kw)
        data = buf.getvalue()
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        got = R.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), (i, img.shape, kind, kw, int((got != want).sum()))
        n += 1
    assert n == 40
