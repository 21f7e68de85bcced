#!/bin/bash
# Build libfdn_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).  The code object of csrc/lowlight.hip is linked into
# libfdn_lowlight.so beside it, which libfdn_hip.so names as a dependency (found through $ORIGIN): callers load and link
# libfdn_hip.so alone and find every entry point there, while its own code objects, the subject of tests/kernel_table.txt, stay
# what they were (tests/kernel_table_lowlight.txt is the table of the dependency).
#   OUT=path BUILD=dir EXTRA="flags" ./build.sh   builds a variant elsewhere (A/B experiments)
set -e
cd "$(dirname "$0")"
OUT=${OUT:-fdn_hip/libfdn_hip.so}
BUILD=${BUILD:-build}
mkdir -p fdn_hip "$BUILD"
# The SLP vectoriser pairs fp32 ops into v_pk_* at the price of v_mov shuffles and ~45 more VGPRs; the
# VALU-issue-bound kernels listed here measure faster without it (fdffn_mid 2.35 -> 1.89 ms at level 1).
NOSLP="patchfft ffn_tail fdsa_full"
OBJS=""
SEPARATE="lowlight"                                   # linked into $(dirname $OUT)/libfdn_<name>.so, a dependency of $OUT
PIDS=""
NEWEST_HDR=$(ls -t csrc/*.hpp csrc/*.inc ../include/fdn_hip.h ../include/fdn_video.h ../include/fdn_temporal.h ../include/fdn_vmetrics.h ../include/fdn_ensemble.h ../include/fdn_spectral.h ../include/fdn_lowlight.h build.sh | head -1)
for f in csrc/*.hip; do
  n=$(basename "${f%.hip}")
  o=$BUILD/$n.o
  fl=""
  for k in $NOSLP; do [ "$k" = "$n" ] && fl="-fno-slp-vectorize"; done
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ "$NEWEST_HDR" -nt "$o" ]; then
    rm -f "$o"                      # a failed compile must not leave a stale object for the link below
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $fl $EXTRA -c "$f" -o "$o" &
    PIDS="$PIDS $!"
  fi
  case " $SEPARATE " in *" $n "*) ;; *) OBJS="$OBJS $o" ;; esac
done
for p in $PIDS; do wait "$p" || { echo "build.sh: a hipcc job failed" >&2; exit 1; }; done
DEPS=""
for n in $SEPARATE; do
  d="$(dirname "$OUT")/libfdn_$n.so"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libfdn_$n.so -o "$d" "$BUILD/$n.o"
  echo "built $d"
  DEPS="$DEPS $d"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-as-needed -Wl,-rpath,'$ORIGIN' -o "$OUT" $OBJS $DEPS
echo "built $OUT"
