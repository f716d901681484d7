# Runs ON the GPU box: everything behind the round's committed profiles (GPU test log, kernel trace + PMC passes of the bench step, the VAE
# passes in the default f16x3 mode, the `--full` bench line, the end-to-end clip times, the default-workload tuning sweep).
# usage: final_profiles.sh [quick]   (quick: tests, DiT profiles and the bench line only)
# Logs and traces go under $OUT (default profile_out/; tools/vae_profiles.sh keeps its own output folder).
export OUT=${OUT:-profile_out}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
mkdir -p "$OUT"
python -m pytest tests -m gpu -q --durations=8 > "$OUT/pytest_gpu_full.log" 2>&1; tail -14 "$OUT/pytest_gpu_full.log" > "$OUT/pytest_gpu.log"
bash tools/collect_profiles.sh
( time python3 bench.py --full ) > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
if [ "$1" != "quick" ]; then
  bash tools/vae_profiles.sh f16x3 both
  python3 tools/end_to_end.py > "$OUT/end_to_end.log" 2>&1
  python3 tools/default_shape_tune.py > "$OUT/default_shape_tune.log" 2>&1
fi
tail -3 "$OUT/pytest_gpu.log"; tail -3 "$OUT/bench_default.err"
