set -x
T=${1:-r06}
OUT=${OUT:-run_out}; mkdir -p $OUT
python -m pytest tests -m gpu -q 2>&1 | tail -8 > $OUT/${T}_gputest_final.log; tail -3 $OUT/${T}_gputest_final.log
profiles/run_profile.sh $T > $OUT/${T}_run_profile.log 2>&1; tail -5 $OUT/${T}_run_profile.log
profiles/pmc_busy.sh $T > $OUT/${T}_pmc_busy.txt 2>&1
profiles/pmc_dyn.sh $T 8192 > $OUT/${T}_pmc_dyn.txt 2>&1
profiles/timeline_call.sh $T 128 > $OUT/${T}_timeline_128.txt 2>&1
python profiles/parity_report.py > $OUT/${T}_parity_report.txt 2>&1; tail -5 $OUT/${T}_parity_report.txt
python profiles/latency_probe.py > $OUT/${T}_latency_probe.txt 2>&1; tail -5 $OUT/${T}_latency_probe.txt
python profiles/debug/refill_probe.py 8192 4096 2048 1024 > $OUT/${T}_refill_probe.txt 2>&1
( time python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${T}_bench_final.json 2> $OUT/${T}_bench_final.err ) 2>&1 | tail -3
cp bench_detail.json $OUT/${T}_bench_detail.json
tail -c 300 $OUT/${T}_bench_final.json
