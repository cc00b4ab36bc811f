set -e
R=$PWD
O=$(realpath -m "${1:?usage: bash tools/profile_round.sh OUT_DIR}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/bench -- python3 $R/bench.py --full --no-cpu-baseline > $O/bench_prof_line.json 2>$O/bench_prof.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/fir -- python3 $R/tools/bench_fir.py > $O/fir.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stress -- python3 $R/tools/bench_stress.py 128 > $O/stress.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/fast -- python3 $R/tools/bench_fast.py > $O/fast.txt 2>&1
cd $R
python bench.py --full > $O/bench_line.json 2>$O/bench.err
python bench.py --full --two-kernel --no-cpu-baseline > $O/bench_line_two_kernel.json 2>>$O/bench.err
python bench.py --full --bf16 --no-cpu-baseline > $O/bench_line_bf16.json 2>>$O/bench.err
find $O -name "*kernel_trace.csv" -size +20M -delete
ls -R $O | head -40
