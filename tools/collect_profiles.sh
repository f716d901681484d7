# Runs on the MI355X: rocprofv3 kernel trace of the bench command (`--full`, for the eager forward pair behind the timed steps) and the two PMC passes
# for HBM-side traffic. Output under $OUT/prof_* (OUT defaults to profile_out/); summarise with tools/prof_summary.py and commit the summaries under profiles/.
OUT=${OUT:-profile_out}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
mkdir -p "$OUT" && rm -rf "$OUT/prof_kt" "$OUT/prof_fetch" "$OUT/prof_write"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_kt" -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-vae --no-stress-shape --no-default-shape --no-pipeline-path --no-ranker > "$OUT/prof_kt.log" 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/prof_fetch" -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-vae --no-stress-shape --no-default-shape --no-pipeline-path --no-ranker --layers 2 > "$OUT/prof_fetch.log" 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/prof_write" -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-vae --no-stress-shape --no-default-shape --no-pipeline-path --no-ranker --layers 2 > "$OUT/prof_write.log" 2>&1
tail -1 "$OUT/prof_kt.log" | cut -c1-200
# keep the merged output small: the kernel trace CSV of the stats run, the two counter CSVs
find "$OUT/prof_kt" -name "*.csv" ! -name "*kernel_trace.csv" ! -name "*kernel_stats.csv" -delete
find "$OUT/prof_fetch" "$OUT/prof_write" -name "*.csv" ! -name "*counter_collection.csv" -delete
du -sh "$OUT"/prof_*
