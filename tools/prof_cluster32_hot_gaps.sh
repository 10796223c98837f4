# rocprofv3 passes behind the counter section of profiles/r10_cluster32_hot_gaps.md, written as profiles/r10_cluster32_hot_gaps_prof.md.  Run on a GPU
# machine from the repository root: bash tools/prof_cluster32_hot_gaps.sh [OUT_DIR]; OUT_DIR receives copies of the bench line, the trace log and the two records.
# lstm_cluster32.hip with branch-free gather pieces and the one-store flag raise in its long-window steady-state sections (same passes as
# tools/prof_cluster32_xspan.sh, whose record stays that of its own object): the long-window instantiation is `<256, 2, 32, false, 3>` for I <= 24 and
# `<..., false, 4>` above; the kernel is named by their common prefix, which bench.py's lookup in
# profiles/traffic_latest.json also matches.  Every pass runs under its own time limit and the chain stops at the first failure; counters are
# collected in runs of their own (no --pmc beside any other tracing).
set -e
R=$PWD
P=${TMPDIR:-/tmp}/prof_c32h
OUT=${1:-$P/out}
mkdir -p $OUT
B="python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $P/trace -- python3 bench.py --steps 200 --warmup 50 --no-cpu-baseline > $OUT/prof_c32h_bench.json 2> $OUT/prof_c32h_trace.log
echo trace done
timeout -k 10 240 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $P/fetch -- $B > /dev/null 2>&1
timeout -k 10 240 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $P/write -- $B > /dev/null 2>&1
echo traffic done
timeout -k 10 240 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_F32 -d $P/mfma -- $B > /dev/null 2>&1
timeout -k 10 240 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU_MFMA_MOPS_F16 -d $P/mfma16 -- $B > /dev/null 2>&1
timeout -k 10 240 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY -d $P/wave -- $B > /dev/null 2>&1
echo counters done
python3 tools/summarize_prof.py r10_cluster32_hot_gaps_prof $P/trace $P/fetch $P/write "ape_lstm_cluster32<256, 2, 32, false" 65536 1024 --model pocket --T 64 \
    --pmc-dir $P/mfma --pmc-dir $P/mfma16 --pmc-dir $P/wave \
    --source csrc/lstm_cluster32.hip --lds 157712 --flop-per-launch 1.06039345152e11 --peak-tflops 157.3 --skip-first 90 --min-us 200 \
    --note "Command (MI355X, one GPU): \`rocprofv3 --kernel-trace --stats -- python3 bench.py --steps 200 --warmup 50 --no-cpu-baseline\` (launches 91..290 of the 1024 x 64 shape are the timed ones); counters from separate \`--kernel-trace --pmc\` passes of \`bench.py --steps 20 --warmup 5 --no-cpu-baseline\` (FETCH_SIZE; WRITE_SIZE; SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_F32; SQ_INSTS_VALU_MFMA_MOPS_F16; SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY); recipe \`tools/prof_cluster32_hot_gaps.sh\`, summarised on the GPU box by \`tools/summarize_prof.py\`. The peak and MfmaUtil are stated against the f32 matrix peak (157.3 TFLOP/s) like every earlier cluster32 profile; the recurrent products run on f16 MFMAs."
cp profiles/r10_cluster32_hot_gaps_prof.md $OUT/r10_cluster32_hot_gaps_prof.md
cp profiles/traffic_latest.json $OUT/traffic_latest.json
