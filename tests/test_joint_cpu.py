"""Joint marginals without a device (apemost_amd/joint.py): Joint.from_rows equals the restatement of
tests/joint_ref.py on the hand-built rows of tests/summary_rows.py, its projections are the run summary's histograms,
the files round-trip, and the covariance about the first sample holds the accuracy its design claims against exact
rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

from apemost_amd.joint import Joint, all_pairs, tri_index
from apemost_amd.summary import RunSummary, edges
from tests import summary_rows as sr
from tests.joint_ref import RefJoint, assert_equals, same_floats

CHAINS = [0, 1, 2, 299]


def _lo_hi(boxes):
    return np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])


@pytest.fixture(scope="module")
def hand_built():
    """(kept rows, boxes) per (box set, nbins); built once"""
    out = {}
    for box_set in ("A", "B"):
        for nbins in (1, 37, 200):
            rows, boxes = sr.build_rows(box_set, nbins)
            out[box_set, nbins] = (rows[sr.kept_steps()][:, CHAINS], boxes)
    return out


@pytest.mark.parametrize("box_set", ["A", "B"])
@pytest.mark.parametrize("nbins", [1, 37, 200])
def test_from_rows_equals_the_restatement(hand_built, box_set, nbins):
    kept, boxes = hand_built[box_set, nbins]
    lo, hi = _lo_hi(boxes)
    chains = list(range(len(CHAINS)))
    got = Joint.from_rows(kept, lo, hi, chains=chains, nbins=nbins)
    ref = RefJoint(kept, boxes, chains, nbins)
    assert_equals(got, ref, finite_chains=(1, 2, 3), what="%s/%d" % (box_set, nbins))   # chains 1, 2 and 299: finite rows
    assert int(ref.counts.sum()) > 0
    assert got.pairs.tolist() == [list(p) for p in all_pairs(4)] and len(got.pairs) == 6


@pytest.mark.parametrize("nbins", [1, 37, 200])
def test_projections_are_the_summary_histograms(nbins):
    rng = np.random.default_rng(3)
    lo, hi = np.array([0.1, 10.0, -7.3, 0.0]), np.array([50.0, 12.0, -0.2, 0.3])
    rows = np.zeros((5000, 2, 6))
    rows[:, :, :4] = lo + (hi - lo) * rng.uniform(0, 1, (5000, 2, 4))
    rows[:50, :, :4] = hi                                    # the top of the box lies in the widened last bin
    rows[50:100, :, :4] = lo
    jt = Joint.from_rows(rows, lo, hi, chains=(0, 1), nbins=nbins)
    rs = RunSummary.from_rows(rows, 2, nbins, 1, 5000, lo, hi)
    for k in range(2):
        for q, (i, j) in enumerate(jt.pairs.tolist()):
            assert np.array_equal(jt.marginal(k, q, 0), rs.hist[k, i]), (k, i, j)
            assert np.array_equal(jt.marginal(k, q, 1), rs.hist[k, j]), (k, i, j)
            assert int(jt.counts[k, q].sum()) == 5000
    assert np.array_equal(jt.edges(2), edges(-7.3, -0.2, nbins))
    ex, ey, dens = jt.density(0, 0)
    area = (hi[0] - lo[0]) / nbins * (hi[1] - lo[1]) / nbins
    assert abs(dens.sum() * area - 1) < 1e-12 and len(ex) == len(ey) == nbins + 1


def test_files_round_trip(tmp_path, hand_built):
    kept, boxes = hand_built["A", 37]
    lo, hi = _lo_hi(boxes)
    jt = Joint.from_rows(kept[:, 1:3], lo, hi, chains=(0, 1), nbins=37, pairs=[(0, 3), (1, 2), (0, 1)], thin=3)
    jt.chains[:] = (4, 9)
    jt.write(str(tmp_path / "joint.bin"))
    back = Joint.read(str(tmp_path / "joint.bin"))
    for f in ("n", "counts", "origin", "sum", "cross", "pairs", "lo", "hi", "chains"):
        assert getattr(back, f).tobytes() == getattr(jt, f).tobytes() and getattr(back, f).shape == getattr(jt, f).shape, f
    assert back.nbins == 37 and back.thin == 3
    raw = (tmp_path / "joint.bin").read_bytes()
    assert raw[:8] == b"APEMOSTJ" and len(raw) == 48 + 4 * 2 + 4 * 6 + 8 * (2 * 4 + 2 * 2 * 4 + 2 * 10) + 8 * 2 * 3 * 37 * 37
    (tmp_path / "bad.bin").write_bytes(b"APEMOSTS" + raw[8:])
    with pytest.raises(ValueError):
        Joint.read(str(tmp_path / "bad.bin"))
    (tmp_path / "short.bin").write_bytes(raw[:-8])
    with pytest.raises(ValueError):
        Joint.read(str(tmp_path / "short.bin"))

    names = ["a", "b", "c", "d"]
    jt.write_text(tmp_path, names, k=1)
    assert sorted(f.name for f in tmp_path.iterdir() if f.suffix in (".joint", ".matrix")) == [
        "a-b.joint", "a-d.joint", "b-c.joint", "correlation.matrix"]
    text = (tmp_path / "a-d.joint").read_text()
    blocks = text.split("\n\n")
    assert blocks[-1] == "" and len(blocks) == 38            # a blank line after each of the 37 x rows
    ex, ey = jt.edges(0), jt.edges(3)
    cells = np.zeros((37, 37), dtype=np.uint64)
    for a, block in enumerate(blocks[:-1]):
        lines = block.split("\n")
        assert len(lines) == 37
        for b, line in enumerate(lines):
            x0, x1, y0, y1, c = line.split(" ")
            assert (x0, x1, y0, y1) == ("%.15e" % ex[a], "%.15e" % ex[a + 1], "%.15e" % ey[b], "%.15e" % ey[b + 1])
            cells[a, b] = int(c)
    assert np.array_equal(cells, jt.counts[1, 0])
    lines = (tmp_path / "correlation.matrix").read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    got = np.array([[float(v) for v in l.split("\t")] for l in lines[:4]])
    want = jt.corr(1)
    assert same_floats(np.array([[float("%.15e" % v) for v in row] for row in want]), got)


def test_covariance_about_the_origin_against_exact_arithmetic():
    """a narrow first column (centre 5, width 1e-4): sum(xy) - sum(x) sum(y) / n loses seven digits there, the sums
    about the first sample do not.  The bound is the textbook one of recursive summation, gamma_n = n u / (1 - n u)
    with u = 2^-53, with a factor 4 for the rounded differences, the rounded products and the final operations:
    4 gamma_n (sum |d_i d_j| + sum |d_i| sum |d_j| / n) / (n - 1)."""
    n, rho = 20000, 0.8
    rng = np.random.default_rng(11)
    z = rng.standard_normal((n, 2))
    rows = np.zeros((n, 1, 4))
    rows[:, 0, 0] = 5.0 + 1e-4 * z[:, 0]
    rows[:, 0, 1] = 3.0 + 2.0 * (rho * z[:, 0] + np.sqrt(1 - rho * rho) * z[:, 1])
    jt = Joint.from_rows(rows, [4.0, -20.0], [6.0, 20.0], chains=(0,), nbins=8)
    cov, corr, mean = jt.cov(0), jt.corr(0), jt.mean(0)
    cols = [[Fraction(v) for v in rows[:, 0, p].tolist()] for p in range(2)]
    totals = [sum(c) for c in cols]
    gamma = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    d = [np.abs(rows[:, 0, p] - rows[0, 0, p]) for p in range(2)]
    for i in range(2):
        assert abs(Fraction(float(mean[i])) - totals[i] / n) <= 4 * gamma * float(d[i].sum()) / n + 2.0 ** -52 * 6
        for j in range(2):
            exact = (sum(x * y for x, y in zip(cols[i], cols[j])) - totals[i] * totals[j] / n) / (n - 1)
            err = abs(Fraction(float(cov[i, j])) - exact)
            bound = 4 * gamma * (float((d[i] * d[j]).sum()) + float(d[i].sum()) * float(d[j].sum()) / n) / (n - 1)
            print("cov[%d][%d] = %.17g, error %.3g, bound %.3g" % (i, j, cov[i, j], float(err), bound))
            assert err <= bound, (i, j, float(err), bound)
            assert cov[i, j] == cov[j, i]
    assert abs(corr[0, 1] - rho) <= 5 * (1 - rho * rho) / np.sqrt(n), corr[0, 1]
    assert corr[0, 0] == 1.0 and corr[1, 1] == 1.0 and corr[0, 1] == corr[1, 0]
    assert jt.cross[0, tri_index(2, 0, 1)] == jt.cross_matrix(0)[1, 0]


def test_degenerate_inputs():
    jt = Joint.from_rows(np.zeros((0, 2, 5)), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], chains=(1,), nbins=4, pairs=[])
    assert int(jt.n[0]) == 0 and jt.counts.shape == (1, 0, 4, 4) and np.isnan(jt.corr(0)).all()
    one = Joint.from_rows(np.full((1, 1, 4), 0.5), [0.0, 0.0], [1.0, 1.0], nbins=2)
    assert one.counts[0, 0].tolist() == [[0, 0], [0, 1]] and one.origin.tolist() == [[0.5, 0.5]] and not one.sum.any()
    assert one.correlation_text(0) == "nan\tnan\nnan\tnan\n"
