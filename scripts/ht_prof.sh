# kernel trace of the host-trace bench line: are the 16 MB chunk uploads blit kernels?  bash scripts/ht_prof.sh OUTDIR
out=$(realpath -m ${1:?output directory})
mkdir -p $out
root=$PWD
work=$(mktemp -d)
export TMPDIR=$work
cd $work && timeout -k 10 300 rocprofv3 --kernel-trace -d $out/htprof -o run --output-format csv -- python3 $root/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --c3-segments 0 --c5-log-n 0 --program-steps 0 --programs none --host-steps 3 > $out/htprof.json 2> $out/htprof.err || exit 1
echo ok
