#!/bin/bash
# Builds the clock-probe variant of the library (kernels_gemm.hip with -DSMLU_CLOCK_PROBE, every other
# object from the regular build) into sharedmemsparselu.jl_amd/build_clock/; run on the CPU box, then
#   gpurun -- 'SMLU_LIB=$PWD/sharedmemsparselu.jl_amd/build_clock/libsmlu_clock.so python tools/gemm_clock.py'
# and the same variant of tools/gemm_bench (build_clock/gemm_bench_clock), which also prints the K-loop
# stamps (cycles per slice by segment) of the 128 tile, e.g. for the F22 and the trailing shape:
#   GB_TILES=135 build_clock/gemm_bench_clock 12000,12000,6000; GB_TILES=131 build_clock/gemm_bench_clock 3072,3072,384
set -e
cd "$(dirname "$0")/../sharedmemsparselu.jl_amd"
make -s -j8 libsmlu.so
mkdir -p build_clock
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -Wall -Wno-unused-result --offload-arch=gfx950 -munsafe-fp-atomics \
  -DSMLU_CLOCK_PROBE -c csrc/kernels_gemm.hip -o build_clock/kernels_gemm.o
/opt/rocm/bin/hipcc -shared -fPIC -Wl,-z,defs --offload-arch=gfx950 -o build_clock/libsmlu_clock.so \
  $(ls build/*.o | grep -v -e kernels_gemm -e _bench) build_clock/kernels_gemm.o
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -x hip --offload-arch=gfx950 -munsafe-fp-atomics \
  -DSMLU_CLOCK_PROBE -c tools/gemm_bench.cpp -o build_clock/gemm_bench.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -o build_clock/gemm_bench_clock build_clock/gemm_bench.o \
  build/kernels_front.o build_clock/kernels_gemm.o build/kernels_solve.o
