#!/bin/bash
# Diagnostic: the measurement passes behind profiles/roundN (run on the GPU box from the repo root: bash tools/profile_round.sh <outdir>)
#   the default bench line, rocprofv3 kernel-trace stats of the same command, then separate --pmc passes (never combined with other
#   trace domains), the in-kernel phase shares, the other workloads / variants
out=${1:-gpurun_out/prof}
export TMPDIR=/tmp
mkdir -p $out
python3 bench.py --full --steps 10 --warmup 3 > $out/bench_default.json 2> $out/bench_default.err
rocprofv3 --kernel-trace --stats -d $out/prof -o r --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras > $out/bench_under_rocprof.json 2> $out/rocprof.err
rocprofv3 --kernel-trace --stats -d $out/prof_f32 -o r --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras --arith f32 > $out/bench_f32_under_rocprof.json 2>> $out/rocprof.err
rocprofv3 --kernel-trace --stats -d $out/prof_b512 -o r --output-format csv -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extras --batch 512 > $out/bench_b512_under_rocprof.json 2>> $out/rocprof.err
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $out/pmc_fetch -o f --output-format csv -- python3 tools/kbench.py attn_bwd attn_fwd ffn_fwd ffn_bwd --arith both --reps 2 > $out/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $out/pmc_write -o w --output-format csv -- python3 tools/kbench.py attn_bwd attn_fwd ffn_fwd ffn_bwd --arith both --reps 2 > $out/pmc_write.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_MFMA SQ_WAVE_CYCLES SQ_WAIT_ANY GRBM_GUI_ACTIVE --kernel-trace -d $out/pmc_mfma -o m --output-format csv -- python3 tools/kbench.py attn_bwd attn_fwd ffn_fwd ffn_bwd --arith both --reps 2 > $out/pmc_mfma.log 2>&1
python3 tools/pmc_summary.py traffic $out/pmc_fetch $out/pmc_write > $out/traffic_pmc.json
python3 tools/pmc_summary.py busy $out/pmc_mfma > $out/pmc_busy.json
python3 tools/phase_profile.py > $out/phase_shares.txt 2>&1
for wl in mltag_like_K10_d16_B256 kkbox_like_F13_K10_d64_B4096 tmall_like_F8_K30_d64_h32_B4096 kkbox_real_F13_K5_d40_B4096 synthetic_F40_V100M_K10_d64_B1024; do
  python3 bench.py --full --workload $wl --no-cpu-baseline --no-extras > $out/bench_$wl.json 2> $out/bench_$wl.err
done
for m in RAT_m0 RAT_m1 RAT_m3; do python3 bench.py --full --model $m --no-cpu-baseline --no-extras > $out/bench_$m.json 2> $out/bench_$m.err; done
python3 bench.py --full --no-cpu-baseline --no-extras --no-graph > $out/bench_nograph.json 2> /dev/null
python3 bench.py --full --no-cpu-baseline --no-extras --embedding-grad sorted > $out/bench_sorted.json 2> /dev/null
find $out -name "*kernel_stats.csv" | head
ls $out
