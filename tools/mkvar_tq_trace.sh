#!/bin/bash
# usage: mkvar_tq_trace.sh [name] : builds orbit-2_amd/lib/alt/<name>.so (default tqtrace) with gemm.hip and attn.hip recompiled under
# -DO2_TQ_TRACE (csrc/tail_queue.h: per-workgroup start / end / XCC id of the one-workgroup-per-CU kernels; tools/tail_idle.py reads
# them); the other objects are reused from the last build
set -e
name=${1:-tqtrace}
R=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
T=${TMPDIR:-/tmp}/var_$name
mkdir -p $T $R/orbit-2_amd/lib/alt
for s in gemm attn; do
  $HIPCC --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-result -DO2_TQ_TRACE -c $R/orbit-2_amd/csrc/$s.hip -o $T/$s.o &
done
wait
objs=""
for f in $R/orbit-2_amd/build/*.o; do b=$(basename $f); [ "$b" = gemm.o ] || [ "$b" = attn.o ] || objs="$objs $f"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $R/orbit-2_amd/lib/alt/$name.so $T/gemm.o $T/attn.o $objs
echo built $name
