#!/bin/bash
# development: build a diagnostic variant of the HIP module (in-kernel stamps) for ONE translation unit.
# usage: tools/build_diag.sh gemv_q4k                     (-DGEMV_DIAG=1, the decode GEMVs' stamps: tools/gemv_stamps.py, gemv_wgs.py)
#        tools/build_diag.sh gemm_wide_k4 -DGEMM_DIAG=3   (the wide body: tools/wide_stamps.py)
#        tools/build_diag.sh gemm_lw -DGEMM_DIAG=4        (the loader-wave body: tools/lw_stamps.py)
#        tools/build_diag.sh gemm_ks -DGEMM_DIAG=6        (the K-split-waves body: tools/ks_stamps.py)
#        tools/build_diag.sh gemm_i8 -DGEMM_DIAG=7        (the int8 body: tools/i8_stamps.py)
#        tools/build_diag.sh gemm_lf -DLF_STAMPS=1        (the Q8_0 batch body: tools/lf_stamps.py)
#        tools/build_diag.sh gemm_kr -DKR_BOUNDS=1        (no stamps: every global access of gemm_kr checked, lfamd_debug_kr_oob)
# ONE unit at a time: every stamped unit exports the same reader, lfamd_debug_stamps(dst, n) (csrc/diag_stamps.h).
#   -> llamafile_amd/libllamafile_amd_hip_diag.so  (use with LFAMD_HIP_SO=...)
set -e
TU=${1:-gemv_q4k}
shift || true
DEFS=${@:--DGEMV_DIAG=1}
cd "$(dirname "$0")/../llamafile_amd/csrc"
make -s -j8
mkdir -p diag
EXTRA=""
case $TU in
  gemv_*) EXTRA="-mllvm -amdgpu-kernarg-preload-count=13" ;;
  gemm_*) EXTRA="-fno-slp-vectorize" ;;
esac
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off $EXTRA $DEFS -c $TU.hip -o diag/$TU.o
OBJS=$(ls *.o | grep -v "^$TU.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libllamafile_amd_hip_diag.so diag/$TU.o $OBJS -ldl
echo built ../libllamafile_amd_hip_diag.so
