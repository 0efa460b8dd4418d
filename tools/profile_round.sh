set -x
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/profile_round.sh <output folder, relative to the repository root>}
mkdir -p "$OUT"
timeout 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -2
timeout 600 python bench.py --full > $OUT/bench_r01h.json 2> $OUT/bench_r01h.err
timeout 300 python bench.py --workload C3 --full --no-cpu-baseline > $OUT/bench_r01h_C3.json 2>/dev/null
timeout 300 python bench.py --workload C5 --full --no-cpu-baseline > $OUT/bench_r01h_C5.json 2>/dev/null
timeout 300 python bench.py --workload E2E --steps 5 --warmup 2 > $OUT/bench_r01h_E2E.json 2>/dev/null
timeout 300 python bench.py --workload E2E --steps 5 --warmup 2 --precision f16 > $OUT/bench_r01h_E2E_f16.json 2>/dev/null
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_r01h -o p --output-format csv -- python3 bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-exact-fp32 > $OUT/prof_r01h.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/trf_fetch -o p --output-format csv -- python3 bench.py --steps 4 --warmup 1 --no-cpu-baseline --no-exact-fp32 > $OUT/trf_fetch.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/trf_write -o p --output-format csv -- python3 bench.py --steps 4 --warmup 1 --no-cpu-baseline --no-exact-fp32 > $OUT/trf_write.log 2>&1
python3 tools/pmc_traffic.py $OUT/trf_fetch $OUT/trf_write $OUT/r01h_conv_hbm_traffic.json 1800
timeout 600 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS -d $OUT/spmc1 -o p --output-format csv -- python3 tools/conv_bench.py > $OUT/spmc1.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $OUT/spmc2 -o p --output-format csv -- python3 tools/conv_bench.py > $OUT/spmc2.log 2>&1
python3 tools/pmc_summary.py $OUT/spmc1/p_counter_collection.csv split > $OUT/r01h_split_pmc.txt
python3 tools/pmc_summary.py $OUT/spmc2/p_counter_collection.csv split >> $OUT/r01h_split_pmc.txt
rm -rf $OUT/trf_fetch/p_kernel_trace.csv $OUT/trf_write/p_kernel_trace.csv
ls $OUT/prof_r01h
