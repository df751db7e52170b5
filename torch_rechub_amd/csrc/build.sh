#!/bin/bash
# Builds librechub_hip.so (gfx950 only) in-tree next to the sources.  Usage: build.sh [-j N]
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
INC=../../include
FLAGS="--offload-arch=gfx950 -mcode-object-version=5 -munsafe-fp-atomics -O3 -std=c++17 -fPIC -I$INC -I. -Wall -Wno-unused-function"
mkdir -p _build
pids=()
for src in api.cpp embed.hip cross.hip optim.hip data.hip match.hip fm.hip seqpool.hip mlp.hip din.hip dinmlp.hip crossmix.hip moe.hip linear.hip gemm.hip shard.hip augru.hip ffm.hip interest.hip sine.hip sasrec.hip rq.hip hstu.hip stream_ce.hip session.hip hllm.hip topk.hip ivf.hip twotower.hip t5attn.hip cin.hip metric.hip beam.hip; do
  [ -f "$src" ] || continue
  obj="_build/${src%.*}.o"
  stale=0
  [ -f "$obj" ] || stale=1
  for dep in "$src" *.h $INC/rechub_hip.h; do
    if [ "$dep" -nt "$obj" ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then
    ( $HIPCC $FLAGS -x hip -c "$src" -o "$obj" ) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC _build/*.o -o librechub_hip.so
echo "built $(pwd)/librechub_hip.so"
