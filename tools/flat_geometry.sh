#!/bin/bash
# tools/flat_geometry.sh NAME [HIPCC_FLAGS...] -- builds build/libnafgpu_NAME.so: the product sources with another geometry
# of k_huf_flat (huf_flat.hip: lanes per stream, pieces per lane in flight by output mode), e.g.
#   tools/flat_geometry.sh t64u4 -DNAFGPU_FLAT_THREADS=64 -DNAFGPU_FLAT_UNROLL_ASCII=4
# and prints the registers, scratch and waves per SIMD of its two kernels.  Experiment libraries are timed beside the product
# with NAFGPU_PROBE_LIBS (tools/synth_probe.py, tools/l3_probe.py), at most four per process: each keeps its device buffers.
name=$1; shift
cd "$(dirname "$0")/../nafcodec_amd/csrc" && mkdir -p ../../build || exit 1
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc"
${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS "$@" -S --cuda-device-only -o /dev/null huf_flat.hip -Rpass-analysis=kernel-resource-usage 2>&1 |
    grep -o "VGPRs: [0-9]*\|waves/SIMD\]: [0-9]*\|ScratchSize.*: [0-9]*" | paste -s -d' '
${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS "$@" -shared -o ../../build/libnafgpu_$name.so $(ls *.cpp | grep -v iter_bench) *.hip -lpthread
