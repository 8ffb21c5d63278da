"""Compile check for a user-supplied device likelihood (include/apemost_device_model.h) without a GPU:
the same translation unit the engine hands to hiprtc when a sampler of APEMOST_MODEL_USER is created
(apemost_hip.hip user_model_build) -- '#include "pt_kernels.h"' + the user's file, the four kernels of
each workgroup shape (1, 2, 4, 8 waves per chain) named as template instantiations -- compiled for gfx950 through libhiprtc with ctypes.
With one_barrier (--one-barrier) the one-barrier kernels of APEMOST_HIP_FLAG_USER_ONE_BARRIER are named too.
With analysis (--analysis) it is the second translation unit instead, the one the engine compiles on the first
predict_* or pointwise_* call of such a sampler (user_analysis_build): the same prefix, the user's file, then
'#include "pt_user_fold.h"', whose kernels exist for the optional hooks the file announces (APEMOST_USER_CURVE,
APEMOST_USER_POINTWISE).  Which hooks it has is read off the code object's kernel names, as the engine does.

    python -m apemost_amd.device_model [--one-barrier | --analysis] my_model.hip
"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL_USER, VARIANT = 4, 8   # APEMOST_MODEL_USER, pt_device.h kVariantModel


def _hiprtc():
    for name in ("libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise OSError("libhiprtc.so not found")


OB_WAVES = (4, 8)   # likelihood waves of the one-barrier kernels (pt_kernels.h has_one_barrier)


def ob_kernel_names(km):
    """the one-barrier instantiations user_model_build adds under APEMOST_HIP_FLAG_USER_ONE_BARRIER: the round
    kernel for every kmodel, the calibration kernel for the default proposal law and swap schedule only"""
    names = ["apemost::pt_round_ob_kernel<%d, %d, false, false>" % (km, w) for w in OB_WAVES]
    if km < VARIANT:
        names += ["apemost::pt_calibrate_ob_kernel<%d, %d, false, false>" % (km, w) for w in OB_WAVES]
    return names


# the analysis module's entry points (pt_user_fold.h), by hook
ANALYSIS_KERNELS = {"curve": ("apemost_user_predict_fold", "apemost_user_predict_fold_hist", "apemost_user_predict_curve"),
                    "pointwise": ("apemost_user_pointwise_fold", "apemost_user_pointwise_loglike")}


def hooks_in(blob):
    """the hooks whose kernels a code object of the analysis translation unit holds (a kernel's name is in the
    object's symbol table, terminated by a zero byte)"""
    return tuple(h for h in ("curve", "pointwise") if all(k.encode() + b"\0" in blob for k in ANALYSIS_KERNELS[h]))


def compile_check(path, variant=False, arch="gfx950", one_barrier=False, code=False, analysis=False):
    """-> (ok, compiler log, code bytes); code=True: (ok, log, the code object itself, b"" on failure).
    analysis=True: the analysis translation unit, and a fourth element, the hooks found: a tuple out of
    ("curve", "pointwise"), empty on failure"""
    rtc = _hiprtc()
    src = ('#define APEMOST_USER_MODEL 1\n#include "pt_kernels.h"\n#line 1 "%s"\n%s\n' % (path, open(path).read())).encode()
    if analysis:
        src += b'#include "pt_user_fold.h"\n'
    prog = C.c_void_p()
    if rtc.hiprtcCreateProgram(C.byref(prog), src, b"apemost_user_model.hip", 0, None, None) != 0:
        raise RuntimeError("hiprtcCreateProgram failed")
    km = MODEL_USER + (VARIANT if variant else 0)
    for w in () if analysis else (1, 2, 4, 8):          # the workgroup shapes the engine instantiates (apemost_hip.hip kUserWaves)
        prod = "true" if w >= 4 else "false"
        for name in ("apemost::pt_round_kernel<%d, %d, false, %s>" % (km, w, prod),
                     "apemost::pt_calibrate_kernel<%d, %d, false, %s>" % (km, w, prod),
                     "apemost::pt_calc_model_kernel<%d, %d, false>" % (MODEL_USER, w),
                     "apemost::pt_loglike_kernel<%d, %d, false>" % (MODEL_USER, w)):
            rtc.hiprtcAddNameExpression(prog, name.encode())
    if one_barrier and not analysis:
        for name in ob_kernel_names(km):
            rtc.hiprtcAddNameExpression(prog, name.encode())
    opts = [b"--offload-arch=" + arch.encode(), b"-O3", b"-ffp-contract=off", b"-std=c++17",
            b"-I" + os.path.join(HERE, "csrc").encode(), b"-I" + os.path.join(ROOT, "include").encode(), b"-I/opt/rocm/include"]
    rc = rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts))
    n = C.c_size_t(0)
    rtc.hiprtcGetProgramLogSize(prog, C.byref(n))
    log = C.create_string_buffer(n.value + 1)
    if n.value:
        rtc.hiprtcGetProgramLog(prog, log)
    size = C.c_size_t(0)
    blob = b""
    if rc == 0:
        rtc.hiprtcGetCodeSize(prog, C.byref(size))
        if code or analysis:
            buf = C.create_string_buffer(size.value)
            rtc.hiprtcGetCode(prog, buf)
            blob = buf.raw
    rtc.hiprtcDestroyProgram(C.byref(prog))
    out = (rc == 0, log.value.decode("utf-8", "replace"), blob if code else size.value)
    return out + (hooks_in(blob),) if analysis else out


if __name__ == "__main__":
    ok_all = True
    one_barrier, analysis = "--one-barrier" in sys.argv[1:], "--analysis" in sys.argv[1:]
    for p in [a for a in sys.argv[1:] if a not in ("--one-barrier", "--analysis")]:
        ok, log, size, *hooks = compile_check(p, one_barrier=one_barrier, analysis=analysis)
        found = ", hooks: %s" % (", ".join(hooks[0]) or "none") if analysis and ok else ""
        print("%s: %s%s%s" % (p, "compiles (%d bytes of gfx950 code)" % size if ok else "DOES NOT COMPILE", found,
                              "\n" + log if log.strip() else ""))
        ok_all = ok_all and ok
    sys.exit(0 if ok_all else 1)
