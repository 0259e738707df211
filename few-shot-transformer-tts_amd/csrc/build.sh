#!/bin/bash
# Build libb2s_hip.so and the eight satellite libraries (libb2s_vocoder.so, libb2s_metrics.so, libb2s_mcd.so, libb2s_f0.so, libb2s_dur.so,
# libb2s_pros.so, libb2s_va.so, libb2s_vp.so) for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   build.sh            only what changed
#   build.sh --clean    recompile every source (what __graft_entry__.build() runs)
#   build.sh --lab      measurement build with -DB2S_LAB (B2S_LAB_* environment switches that change results: skip the encoder, drop the
#                       exchange ordering) -> ../../tools/bin/libb2s_hip_lab.so, used through B2S_LIB_PATH; never the product library
set -e
cd "$(dirname "$0")"
OUT=../libb2s_hip.so
OBJ=obj
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
if [ "$1" = "--lab" ]; then OBJ=obj_lab; mkdir -p ../../tools/bin; OUT=../../tools/bin/libb2s_hip_lab.so; FLAGS="$FLAGS -DB2S_LAB"; fi
if [ "$1" = "--clean" ]; then rm -rf $OBJ; fi
mkdir -p $OBJ
SRCS="gemm gemm_glds gemm_glds256 gemm_skinny attention attention32 rowops engine capi_ops decode decode_fused enc_fused"
pids=()
for f in $SRCS; do
  if [ ! -f $OBJ/$f.o ] || [ $f.hip -nt $OBJ/$f.o ] || [ -n "$(find . -maxdepth 1 -name '*.h' -newer $OBJ/$f.o)" ] || [ ../../include/b2s_hip.h -nt $OBJ/$f.o ]; then
    hipcc $FLAGS -c $f.hip -o $OBJ/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
objs=""; for f in $SRCS; do objs="$objs $OBJ/$f.o"; done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $OUT
echo "built $OUT"
# A satellite library: ../libb2s_NAME.so from its sources plus the shared error core (side_common.hip), rebuilt when any of them,
# side_common.h or its header include/b2s_NAME.h is newer.  satellite NAME "EXTRA FLAGS" SOURCE...
MODE=$1
satellite() {
  local out=../libb2s_$1.so header=../../include/b2s_$1.h extra=$2 stale=$MODE f
  shift 2
  local srcs="$* side_common.hip"
  for f in $srcs side_common.h $header; do
    if [ ! -f $out ] || [ $f -nt $out ]; then stale=--clean; fi
  done
  if [ "$stale" = "--clean" ]; then hipcc $FLAGS $extra -shared $srcs -o $out; fi
  echo "built $out"
}
# not part of the measurement build
if [ "$1" != "--lab" ]; then
  # the vocoder / mel front end, silence trimming, corpus preparation and resampling (include/b2s_vocoder.h)
  satellite vocoder "" vocoder/vocoder.hip vocoder/silence.hip vocoder/prep.hip vocoder/resample.hip
  # batched FastDTW / MSE-after-DTW eval metric, alignment-head selection and edit distance (include/b2s_metrics.h)
  satellite metrics "" metrics/dtw.hip metrics/align.hip metrics/edit.hip
  # mel-cepstral distortion after DTW (include/b2s_mcd.h); contraction off, the definition rounds every product and sum on its own
  satellite mcd "-ffp-contract=off" mcd/mcd.hip
  # YIN pitch tracking and the F0 error after DTW (include/b2s_f0.h); contraction off, the exact sums use explicit fma()
  satellite f0 "-ffp-contract=off" f0/f0.hip
  # monotonic alignment search and the duration error (include/b2s_dur.h); contraction off, every cell is one fp64 add and one compare
  satellite dur "-ffp-contract=off" dur/dur.hip
  # prosody targets: window energy, Viterbi pitch track, sums per input unit (include/b2s_pros.h); contraction off, every product is
  # rounded before it is added
  satellite pros "-ffp-contract=off" pros/pros.hip
  # the student's variance adaptor, forward and backward: quantise, embed, expand (include/b2s_va.h); contraction off with the
  # siblings, every sum is one rounded fp32 add after the other
  satellite va "-ffp-contract=off" va/va.hip
  # the student's variance predictors, forward and backward: conv, ReLU, LayerNorm, dropout twice, Linear (include/b2s_vp.h);
  # contraction off, every product outside an explicit fmaf is rounded before it is added
  satellite vp "-ffp-contract=off" vp/vp.hip
fi
