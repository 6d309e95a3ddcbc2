# Collects the rocprofv3 evidence kept under profiles/ (run on the GPU box through gpurun): bench lines, kernel statistics for c2..c5,
# PMC traffic + MFMA utilisation for c2 and c3, the hyper-on iteration.  Outputs land in $O (default prof_out/;
# tools/pmc_traffic.py keeps its own output folder); copy what is to be kept into profiles/.   usage: bash tools/collect_profiles.sh [tag]   (default r03)
export TMPDIR=/tmp
R=$PWD
T=${1:-r04}
O=${O:-prof_out}
mkdir -p $O
python bench.py --full > $O/${T}_c2_bench_line.json 2> $O/${T}_c2_line.err
for c in c3 c4 c5; do
  st=100; wu=20; [ $c = c5 ] && st=20 && wu=5; [ $c = c4 ] && st=60 && wu=10
  python bench.py --config $c --steps $st --warmup $wu --full --cpu-elbo-seconds 0 > $O/${T}_${c}_bench_line.json 2> $O/${T}_${c}_line.err
done
for c in c2 c3 c4 c5; do
  st=100; wu=20; [ $c = c5 ] && st=20 && wu=5; [ $c = c4 ] && st=60 && wu=10
  (cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_${T}_$c -o p -- python $R/bench.py --config $c --steps $st --warmup $wu --no-cpu-baseline --no-elbo-tol --no-extras > /dev/null 2>&1)
  cp $O/prof_${T}_$c/p_kernel_stats.csv $O/${T}_${c}_kernel_stats.csv
done
python tools/step_gaps.py $O/prof_${T}_c2/p_kernel_trace.csv > $O/${T}_c2_step_gaps.txt 2>&1
# the reference's default training mode: hyper-parameter step every iteration
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_${T}_hyper -o p -- python $R/tools/prof_hyper.py > /dev/null 2>&1)
cp $O/prof_${T}_hyper/p_kernel_stats.csv $O/${T}_c2_hyper_kernel_stats.csv
python tools/hyper_timeline.py $O/prof_${T}_hyper/p_kernel_trace.csv > $O/${T}_c2_hyper_timeline.txt 2>&1
python tools/pmc_traffic.py collect c2 ${T}_c2 > /dev/null 2>&1; python tools/pmc_traffic.py parse c2 ${T}_c2 > $O/${T}_pmc_c2.log 2>&1
python tools/pmc_traffic.py collect c3 ${T}_c3 > /dev/null 2>&1; python tools/pmc_traffic.py parse c3 ${T}_c3 > $O/${T}_pmc_c3.log 2>&1
python tools/pmc_traffic.py mfma c2 ${T}_c2 > $O/${T}_mfma_c2.log 2>&1
for c in c2 c3 c4 c5; do echo == $c; python tools/summarize_prof.py $O/${T}_${c}_kernel_stats.csv 8; tail -c 600 $O/${T}_${c}_bench_line.json; echo; done
echo == hyper; python tools/summarize_prof.py $O/${T}_c2_hyper_kernel_stats.csv 12
cat $O/${T}_pmc_c2.log | head -30
