"""Child process of tests/test_gpu_q80_relaxed.py: one llamafile_sgemm call on HOST pointers through libllamafile_sgemm.so, in a
process of its own because the shim reads LFAMD_Q80_RELAXED once, when it loads the module.  argv: A.npy B.npy out.npy m n k."""
import ctypes as C
import sys

import numpy as np

from llamafile_amd import _hip, ggml_types as T


def main():
    a_path, b_path, out_path, m, n, k = sys.argv[1:4] + [int(v) for v in sys.argv[4:7]]
    A, B = np.load(a_path), np.load(b_path)
    lib = C.CDLL(_hip.HOST_SO)
    lib.llamafile_sgemm.restype = C.c_bool
    lib.llamafile_sgemm.argtypes = [C.c_long] * 3 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long] + [C.c_int] * 5
    lib.llamafile_sgemm_amd_available.restype = C.c_int
    assert lib.llamafile_sgemm_amd_available() == 1
    out = np.full((n, m), np.nan, dtype=np.float32)
    kb = k // 32
    assert lib.llamafile_sgemm(m, n, kb, A.ctypes.data, kb, B.ctypes.data, kb, out.ctypes.data, m, 0, 1, T.Q8_0, T.Q8_0, T.F32)
    np.save(out_path, out)


if __name__ == "__main__":
    main()
