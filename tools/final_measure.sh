export TMPDIR=/tmp; cd "$(dirname "$0")/.."; O=${OUT:-out}; mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q > $O/all6.log 2>&1; echo "pytest rc=$?"; tail -3 $O/all6.log
timeout 300 python -c 'import __graft_entry__ as g; g.smoke()' 2>&1 | tail -3
timeout 600 python bench.py --full > $O/bench6.json 2> $O/bench6.err; cat $O/bench6.json
rm -rf $O/prof6; timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof6 -o p -- python bench.py --no-cpu-baseline --no-latency > $O/bench6_prof.json 2> $O/prof6.err; cat $O/bench6_prof.json; head -12 $O/prof6/p_kernel_stats.csv
timeout 900 bash tools/hbm_traffic.sh
timeout 600 bash tools/mfma_util.sh
