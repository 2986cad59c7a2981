#!/bin/bash
# end-of-round evidence: bench lines (default / fp32 UNet / SSIM), rocprofv3 kernel-trace summaries (two decoder streams and
# single stream), PMC traffic.  The PMC passes land where tools/pmc_traffic.sh puts them, everything else under $PROFILE_OUT
# (default profile_out/); copy what is to be judged into profiles/.
#   tools/profile_round.sh r02_g
tag=${1:-r04}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
PMC_TAG=${PMC_TAG:-r04} bash tools/pmc_traffic.sh          # first: bench.py quotes roofline.traffic from the summary of THIS build (csrc hash)
out=${PROFILE_OUT:-profile_out}
mkdir -p $out
python3 bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
python3 bench.py --full --model unet --precision fp32 --batch 16 --no-cpu-baseline > $out/${tag}_bench_unet_fp32.json 2>> $out/${tag}_bench.err
python3 bench.py --full --ssim --no-cpu-baseline > $out/${tag}_bench_ssim.json 2>> $out/${tag}_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -- python3 bench.py --full --steps 20 --warmup 5 --blocks 1 --no-cpu-baseline > $out/${tag}_profiled_bench.json 2> $out/${tag}_prof.err
UNET_TWO_STREAMS=0 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof1 -- python3 bench.py --full --steps 20 --warmup 5 --blocks 1 --no-cpu-baseline > $out/${tag}_profiled1_bench.json 2> $out/${tag}_prof1.err
find $out/${tag}_prof $out/${tag}_prof1 -name "*kernel_stats.csv" | while read f; do cp $f $out/$(echo ${f#$out/} | cut -d/ -f1)_kernel_stats.csv; done
find $out/${tag}_prof $out/${tag}_prof1 -name "*kernel_trace.csv" -delete
ls $out | grep ${tag}
