# Wall time of the whole --full bench run.  usage: tools/time_bench.sh <output directory>
out=${1:?usage: tools/time_bench.sh <output directory>}; mkdir -p "$out"
S=$(date +%s); python bench.py --full > "$out/bench_full.log" 2> "$out/bench_full.err"; echo "rc $? elapsed $(( $(date +%s) - S )) s"
