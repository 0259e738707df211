#!/bin/bash
# Build libb2s_hip.so, libb2s_vocoder.so, libb2s_metrics.so and libb2s_mcd.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
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
# the vocoder / mel front end is a library of its own (include/b2s_vocoder.h); not part of the measurement build
if [ "$1" != "--lab" ]; then
  VOUT=../libb2s_vocoder.so
  if [ "$1" = "--clean" ] || [ ! -f $VOUT ] || [ vocoder/vocoder.hip -nt $VOUT ] || [ vocoder/silence.hip -nt $VOUT ] || [ vocoder/prep.hip -nt $VOUT ] || [ vocoder/resample.hip -nt $VOUT ] || [ ../../include/b2s_vocoder.h -nt $VOUT ]; then
    hipcc $FLAGS -shared vocoder/vocoder.hip vocoder/silence.hip vocoder/prep.hip vocoder/resample.hip -o $VOUT
  fi
  echo "built $VOUT"
  # batched FastDTW / MSE-after-DTW eval metric, alignment-head selection and edit distance: a library of its own too (include/b2s_metrics.h)
  MOUT=../libb2s_metrics.so
  if [ "$1" = "--clean" ] || [ ! -f $MOUT ] || [ metrics/dtw.hip -nt $MOUT ] || [ metrics/align.hip -nt $MOUT ] || [ metrics/edit.hip -nt $MOUT ] || [ metrics/met_common.h -nt $MOUT ] || [ ../../include/b2s_metrics.h -nt $MOUT ]; then
    hipcc $FLAGS -shared metrics/dtw.hip metrics/align.hip metrics/edit.hip -o $MOUT
  fi
  echo "built $MOUT"
  # mel-cepstral distortion after DTW: the cepstral front end and the scoring along the path (include/b2s_mcd.h); contraction off,
  # the definition rounds every product and sum on its own
  COUT=../libb2s_mcd.so
  if [ "$1" = "--clean" ] || [ ! -f $COUT ] || [ mcd/mcd.hip -nt $COUT ] || [ ../../include/b2s_mcd.h -nt $COUT ]; then
    hipcc $FLAGS -ffp-contract=off -shared mcd/mcd.hip -o $COUT
  fi
  echo "built $COUT"
fi
