#!/bin/bash
# The round's closing measurements on ONE box (run from the repo root on the GPU box): tools/profile_round.sh <tag f32> <tag bf16> <outdir>
# rocprofv3 passes of the 720p fp32 forward and of the 1080p B = 4 bf16 forward (tools/profile_passes.sh), merged summaries,
# then bench.py --full lines for the headline and the other configurations.  Everything lands under <outdir>, a directory relative to the repo root.
A=${1:-r04_n}; B=${2:-r04_o}; O=${3:?usage: tools/profile_round.sh <tag f32> <tag bf16> <outdir>}
mkdir -p "$O"
tools/profile_passes.sh $O/$A > $O/${A}_passes.log 2>&1
python tools/profile_merge.py $O/$A $O/$A > $O/${A}_merge.log 2>&1
tools/profile_passes.sh $O/$B --height 1080 --width 1920 --batch 4 --dtype bf16 > $O/${B}_passes.log 2>&1
python tools/profile_merge.py $O/$B $O/$B > $O/${B}_merge.log 2>&1
rm -rf $O/$A/*/ $O/$B/*/ 2>/dev/null
python bench.py --full --steps 10 --warmup 2 > $O/${A}_bench.json 2> $O/${A}_bench.err
python bench.py --full --steps 10 --warmup 2 --dtype bf16 --no-cpu-baseline > $O/${A}_bench_bf16.json 2>> $O/${A}_bench.err
python bench.py --full --steps 6 --warmup 2 --height 1080 --width 1920 --batch 4 --dtype bf16 --no-cpu-baseline > $O/${B}_bench_1080p_bf16.json 2>> $O/${A}_bench.err
python bench.py --full --steps 6 --warmup 2 --height 1080 --width 1920 --batch 4 --no-cpu-baseline > $O/${B}_bench_1080p_f32.json 2>> $O/${A}_bench.err
head -3 $O/${A}_summary.txt; head -3 $O/${B}_summary.txt
