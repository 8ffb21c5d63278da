"""A numpy restatement of the reference's peaks.exe (tools/peaks.c, `peaks.exe min max file`), held to recorded
runs of the compiled tool (tests/golden/peaks/<case>/, tests/test_peaks_cpu.py).  It shares nothing with the device
code or with apemost_hip_peaks_table: the tests compare both against it with ==.

  1. filter  tools/peaks.c:101    v >= min && v <= max, both ends inclusive; NaN is dropped
  2. sort    :147                 ascending as numbers
  3. cut     :151, :161-188       gap = (max - min) / 100; a peak starts at sorted index i when v[i] - v[i-1] > gap
  4. select  :56-80               n = right - left + 1; c <= n*j/4 picks v[left + n*j/4 - 1] for j = 1, 2, 3; where
                                  n*j/4 is 0 the variable keeps what the peak before left in it (:130: they live in
                                  run() and start at 0)
  5. share   :63                  1.0 * n / nvalues
  6. order   src/gsl_helper.c:102-127  selection sort, descending by share, strict >, rows j and best swapped
  7. print   :194-201             "median\\t-\\t+\\tpercent\\n", then "%f\\t%f\\t%f\\t%f\\n" of median, median - left
                                  quartile, right quartile - median, share
With no admitted value the result is the header alone (the tool reads uninitialised memory there).
"""
import numpy as np

PEAKS_MAX = 99
HEADER = "median\t-\t+\tpercent\n"


class RefPeaks:
    """one column: every field of the device's view, the table and the text"""

    def __init__(self, values, lo, hi):
        v = np.asarray(values, dtype=np.float64)
        lo, hi = float(lo), float(hi)
        with np.errstate(invalid="ignore"):
            kept = v[(v >= lo) & (v <= hi)]                                  # 1
        s = np.sort(kept)                                                    # 2
        self.sorted = s
        self.n_values = len(s)
        gap = (hi - lo) / 100                                                # 3
        starts = ([0] + (np.nonzero(s[1:] - s[:-1] > gap)[0] + 1).tolist()) if len(s) else []
        self.n_peaks = len(starts)
        ends = [b - 1 for b in starts[1:]] + ([len(s) - 1] if len(s) else [])
        self.left = np.zeros(PEAKS_MAX, dtype=np.uint64)
        self.right = np.zeros(PEAKS_MAX, dtype=np.uint64)
        self.q = np.zeros((PEAKS_MAX, 3))
        self.q_set = np.zeros(PEAKS_MAX, dtype=np.uint8)
        stat = [0.0, 0.0, 0.0]                                               # left quartile, median, right quartile
        rows = []
        for c, (left, right) in enumerate(zip(starts, ends)):
            n = right - left + 1
            for j in range(3):                                               # 4
                count = n * (j + 1) // 4
                if count >= 1:
                    stat[j] = float(s[left + count - 1])
                    if c < PEAKS_MAX:
                        self.q[c, j] = stat[j]
                        self.q_set[c] |= 1 << j
            if c < PEAKS_MAX:
                self.left[c], self.right[c] = left, right
            rows.append([1.0 * n / self.n_values, stat[1], stat[0], stat[2]])   # 5: share, median, left, right
        for j in range(len(rows)):                                           # 6
            best = j
            for i in range(j + 1, len(rows)):
                if rows[i][0] > rows[best][0]:
                    best = i
            if j != best:
                rows[j], rows[best] = rows[best], rows[j]
        self.table = np.array([[r[1], r[1] - r[2], r[3] - r[1], r[0]] for r in rows]).reshape(len(rows), 4)
        self.text = HEADER + "".join("%f\t%f\t%f\t%f\n" % tuple(r) for r in self.table.tolist())   # 7
