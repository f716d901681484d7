# Runs ON the GPU box: SQ / GRBM counters of every kernel of a 2-block denoise step (effective clock and MFMA-pipe occupancy per kernel).
# Output under $OUT/pmc_step (OUT defaults to profile_out/).
OUT=${OUT:-profile_out}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
mkdir -p "$OUT" && rm -rf "$OUT/pmc_step"
rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES --output-format csv -d "$OUT/pmc_step" -- python3 bench.py --full --steps 2 --warmup 2 --no-cpu-baseline --no-vae --no-pipeline-path --no-ranker --layers 4 > "$OUT/pmc_step.log" 2>&1
find "$OUT/pmc_step" -name "*.csv" ! -name "*counter_collection.csv" ! -name "*kernel_trace.csv" -delete
du -sh "$OUT/pmc_step"
