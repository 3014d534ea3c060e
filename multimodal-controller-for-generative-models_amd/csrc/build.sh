#!/bin/bash
# Builds libmcgen_hip.so for gfx950 in-tree (cross-compiles without a GPU).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable ${MCGEN_EXTRA_FLAGS:-}"
mkdir -p build
pids=()
for f in conv_fused conv_skinny conv_smap conv_px1 conv_c8 conv_head wgrad wgrad_multi wgrad_c8 small_ops glow_ops pixelcnn_ops vq_ops classifier_ops pixelcnn_sample cgan_ops cpixelcnn_ops cvae_ops cglow_ops glow_variants dbi_ops eval_ops score_ops optim_ops ema_ops; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ mcgen_common.h -nt build/$f.o ] || [ conv_tile.h -nt build/$f.o ] || [ ../../include/mcgen_hip.h -nt build/$f.o ]; then
    $HIPCC $FLAGS -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libmcgen_hip.so build/conv_fused.o build/conv_skinny.o build/conv_smap.o build/conv_px1.o build/conv_c8.o build/conv_head.o build/wgrad.o build/wgrad_multi.o build/wgrad_c8.o build/small_ops.o build/glow_ops.o build/pixelcnn_ops.o build/vq_ops.o build/classifier_ops.o build/pixelcnn_sample.o build/cgan_ops.o build/cpixelcnn_ops.o build/cvae_ops.o build/cglow_ops.o build/glow_variants.o build/dbi_ops.o build/eval_ops.o build/score_ops.o build/optim_ops.o build/ema_ops.o
echo "built $(pwd)/libmcgen_hip.so"
