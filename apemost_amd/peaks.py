"""Peaks: what the reference's peaks.exe prints (tools/peaks.c), from what apemost_hip_peaks_get hands out.

A Peaks object holds one view (include/apemost_hip.h, apemost_hip_peaks_view): per kept chain k and parameter p the
number of values inside [lo[p], hi[p]], the number of peaks -- runs of sorted values with no gap above
(hi - lo) / 100 -- and for each of the first 99 peaks its bounds in the sorted order and the three order statistics
the tool reads out of it.  table() and text() go through apemost_hip_peaks_table, the library's host function: the
carry-over of a statistic that a small peak does not have, the shares and the tool's selection sort are stated once,
in C, for the C host, this class and the tests alike.
"""
import ctypes as C
import os

import numpy as np

from . import capi

HEADER = "median\t-\t+\tpercent\n"


class Peaks:
    def __init__(self, n, n_values, n_peaks, left, right, q, q_set, lo=None, hi=None, chains=None):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.n_values = np.ascontiguousarray(n_values, dtype=np.uint64)          # [k][p]
        self.n_peaks = np.ascontiguousarray(n_peaks, dtype=np.uint32)            # [k][p]
        self.left = np.ascontiguousarray(left, dtype=np.uint64)                  # [k][p][99]
        self.right = np.ascontiguousarray(right, dtype=np.uint64)                # [k][p][99]
        self.q = np.ascontiguousarray(q, dtype=np.float64)                       # [k][p][99][3]
        self.q_set = np.ascontiguousarray(q_set, dtype=np.uint8)                 # [k][p][99]
        self.n_keep, self.n_par = self.n_values.shape
        m = capi.PEAKS_MAX
        assert self.n_peaks.shape == (self.n_keep, self.n_par)
        assert self.left.shape == self.right.shape == self.q_set.shape == (self.n_keep, self.n_par, m)
        assert self.q.shape == (self.n_keep, self.n_par, m, 3)
        self.lo, self.hi, self.chains = lo, hi, chains

    @classmethod
    def empty(cls, n_keep, n_par, lo=None, hi=None, chains=None):
        m = capi.PEAKS_MAX
        return cls(np.zeros(1, dtype=np.uint64), np.zeros((n_keep, n_par), dtype=np.uint64),
                   np.zeros((n_keep, n_par), dtype=np.uint32), np.zeros((n_keep, n_par, m), dtype=np.uint64),
                   np.zeros((n_keep, n_par, m), dtype=np.uint64), np.zeros((n_keep, n_par, m, 3)),
                   np.zeros((n_keep, n_par, m), dtype=np.uint8), lo, hi, chains)

    def view(self):
        """the apemost_hip_peaks_view over this object's arrays"""
        return capi.PeaksView(n=self.n.ctypes.data_as(capi._up), n_values=self.n_values.ctypes.data_as(capi._up),
                              n_peaks=self.n_peaks.ctypes.data_as(C.POINTER(C.c_uint32)),
                              left=self.left.ctypes.data_as(capi._up), right=self.right.ctypes.data_as(capi._up),
                              q=self.q.ctypes.data_as(capi._dp), q_set=self.q_set.ctypes.data_as(C.POINTER(C.c_uint8)))

    def table(self, p, k=0):
        """(n_peaks, 4): median, median - left quartile, right quartile - median, share; largest share first"""
        out = np.zeros((capi.PEAKS_MAX, 4))
        rows = C.c_uint32(0)
        capi.check(capi.lib().apemost_hip_peaks_table(C.byref(self.view()), self.n_par, k, p,
                                                      out.ctypes.data_as(capi._dp), C.byref(rows)))
        return out[:rows.value].copy()

    def text(self, p, k=0):
        """the tool's standard output for this column, byte for byte"""
        return HEADER + "".join("%f\t%f\t%f\t%f\n" % tuple(r) for r in self.table(p, k).tolist())

    def write(self, directory, names, k=0):
        """<name>.peaks for every parameter of kept chain k"""
        assert len(names) == self.n_par
        for p, name in enumerate(names):
            with open(os.path.join(str(directory), name + ".peaks"), "w") as f:
                f.write(self.text(p, k))
