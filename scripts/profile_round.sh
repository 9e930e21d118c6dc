#!/bin/bash
# Round-end profiles: kernel-trace stats + PMC passes (separate runs; never combined with trace domains).
# Usage (on the GPU box): bash scripts/profile_round.sh <tag>
# Output under $PROFILE_OUT (default: profile_out/).
tag=${1:-r02}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=${PROFILE_OUT:-profile_out}
mkdir -p "$O"
rm -rf "$O"/prof_$tag* "$O"/pmc_${tag}_*      # (runs of the same tag overwrite, never mix)
# (long enough for the card to be past its clock ramp for most of the launches: DESIGN.md "How bench.py times")
BENCH="python3 bench.py --steps 200 --warmup 60 --no-cpu-baseline --no-closed-loop --no-extras"
# ---- the bench kernel (BASELINE configs[1])
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$tag -- $BENCH > $O/prof_$tag.json 2> $O/prof_$tag.err
run() { name=$1; shift; rocprofv3 --pmc "$@" --output-format csv -d $O/pmc_${tag}_$name -- python3 bench.py --steps 8 --warmup 2 --no-cpu-baseline --no-closed-loop --no-extras > $O/pmc_${tag}_$name.log 2>&1; }
run sq1 SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES
run sq2 SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_SCA SQ_INSTS_FLAT
run mfma SQ_INSTS_VALU_MFMA_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_BUSY_CU_CYCLES
run fetch FETCH_SIZE
run write WRITE_SIZE
python3 scripts/pmc_summary.py solve_kernel $O/pmc_${tag}_sq1 $O/pmc_${tag}_sq2 $O/pmc_${tag}_mfma $O/pmc_${tag}_fetch $O/pmc_${tag}_write > $O/pmc_${tag}_summary.txt
cat $O/pmc_${tag}_summary.txt
find $O/prof_$tag -name "*kernel_stats.csv" -exec cat {} \; | cut -c1-200 > $O/prof_${tag}_kernel_stats.csv
head -4 $O/prof_${tag}_kernel_stats.csv
# ---- configs[2] (N = 20 extended controller, batch 65536) and configs[4] (n = 12, m = 4, N = 30, batch 16384: block kernel, MFMA)
for cfg in config3 config5; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${tag}_$cfg -- python3 bench.py --full --only $cfg > $O/prof_${tag}_$cfg.json 2> $O/prof_${tag}_$cfg.err
  find $O/prof_${tag}_$cfg -name "*kernel_stats.csv" -exec cat {} \; | cut -c1-200 > $O/prof_${tag}_${cfg}_kernel_stats.csv
  head -4 $O/prof_${tag}_${cfg}_kernel_stats.csv
  rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA --output-format csv -d $O/pmc_${tag}_${cfg}_a -- python3 bench.py --full --only $cfg > $O/pmc_${tag}_${cfg}_a.log 2>&1
  rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT --output-format csv -d $O/pmc_${tag}_${cfg}_b -- python3 bench.py --full --only $cfg > $O/pmc_${tag}_${cfg}_b.log 2>&1
  python3 scripts/pmc_summary.py solve_ $O/pmc_${tag}_${cfg}_a $O/pmc_${tag}_${cfg}_b > $O/pmc_${tag}_${cfg}_summary.txt
  cat $O/pmc_${tag}_${cfg}_summary.txt
done
# ---- the closed loop (tmpc_mc_run): the fused launch (closed_loop_kernel: all T steps of 4096 trajectories) and the launch pair per step, as bench.py times them
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${tag}_closed_loop -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras > $O/prof_${tag}_closed_loop.json 2> $O/prof_${tag}_closed_loop.err
python3 scripts/trace_summary.py $O/prof_${tag}_closed_loop > $O/summ_${tag}_closed_loop_kernel_trace_summary.txt
CL="python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras"
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU --output-format csv -d $O/pmc_${tag}_cl_a -- $CL > $O/pmc_${tag}_cl_a.log 2>&1
rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT --output-format csv -d $O/pmc_${tag}_cl_b -- $CL > $O/pmc_${tag}_cl_b.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_${tag}_cl_f -- $CL > $O/pmc_${tag}_cl_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_${tag}_cl_w -- $CL > $O/pmc_${tag}_cl_w.log 2>&1
python3 scripts/pmc_summary.py closed_loop_kernel $O/pmc_${tag}_cl_a $O/pmc_${tag}_cl_b $O/pmc_${tag}_cl_f $O/pmc_${tag}_cl_w > $O/summ_${tag}_closed_loop_pmc_summary.txt
# summaries written here, on the box, from this run's files only (what gets copied into profiles/)
python3 scripts/trace_summary.py $O/prof_$tag > $O/summ_${tag}_bench_kernel_trace_summary.txt
for cfg in config3 config5; do python3 scripts/trace_summary.py $O/prof_${tag}_$cfg > $O/summ_${tag}_${cfg}_kernel_trace_summary.txt; done
cp $O/pmc_${tag}_summary.txt $O/summ_${tag}_bench_pmc_summary.txt
for cfg in config3 config5; do cp $O/pmc_${tag}_${cfg}_summary.txt $O/summ_${tag}_${cfg}_pmc_summary.txt; done

