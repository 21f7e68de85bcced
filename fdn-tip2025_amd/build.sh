#!/bin/bash
# Build libfdn_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU): every csrc/*.hip, one shared object - but for the files of
# SEPARATE, each linked into a library of its own beside it (csrc/correct.hip -> libfdn_correct.so, which fdn_hip/correct.py loads itself, and
# csrc/sharpness.hip -> libfdn_sharpness.so for fdn_hip/sharpness.py, csrc/fusion.hip -> libfdn_fusion.so for fdn_hip/fusion.py, csrc/motion.hip -> libfdn_motion.so for fdn_hip/motion.py, csrc/mctf.hip -> libfdn_mctf.so for fdn_hip/mctf.py, csrc/piqe.hip -> libfdn_piqe.so for fdn_hip/piqe.py; libfdn_hip.so does not depend on them, and its own code objects, the
# subject of tests/kernel_table.txt, stay what they were).
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
SEPARATE="correct sharpness fusion motion mctf msssim piqe"                   # linked into $(dirname $OUT)/libfdn_<name>.so, not into $OUT
PIDS=""
NEWEST_HDR=$(ls -t csrc/*.hpp csrc/*.inc ../include/*.h build.sh | head -1)
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
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $OBJS
echo "built $OUT"
for n in $SEPARATE; do
  d="$(dirname "$OUT")/libfdn_$n.so"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libfdn_$n.so -o "$d" "$BUILD/$n.o"
  echo "built $d"
done
