set -x
# one round's profile evidence: rocprofv3 stats + PMC of the full bench command, then the bench lines themselves (GPU box)
# usage: scripts/refresh_profiles.sh <tag> [output dir, default profile_out]      -> <output dir>/<tag>/
T=${1:-r06}
D=$(realpath -m ${2:-profile_out})
mkdir -p $D/$T
# the bench lines first, on a box nothing has run on yet (round 6: a sustained run right behind the five rocprofv3 passes read its sampled
# events 20 us long on one box), then the profile passes
python bench.py --full > $D/$T/bench_default.json 2> $D/$T/bench_default.err
python bench.py --steps 20 --warmup 5 > $D/$T/bench_steps20_as_the_driver_runs_it.json 2>/dev/null
bash scripts/profile_round.sh $T default $D > $D/profile_round.log 2>&1
cp $D/prof_$T/kernel_stats.csv $D/prof_$T/pmc_kernels.txt $D/prof_$T/traffic.json $D/$T/ 2>/dev/null
grep -h "^{" $D/prof_$T/trace.log | tail -1 > $D/$T/bench_under_rocprofv3.json
python bench.py --full --workload direct1 --secondary none --no-cpu-baseline --steps 2000 > $D/$T/bench_direct1.json 2>/dev/null
python bench.py --full --decim 512 --no-cpu-baseline --no-other-decim --no-other-specs --secondary none --steps 4000 > $D/$T/bench_decim512.json 2>/dev/null
tail -c 400 $D/$T/bench_default.json
