# Round check on the GPU box: -m gpu suite, full bench line, round profile.
#   bash tools/gpu_round.sh <tag> [tests|bench|prof ...]   (default: all three)
# Logs and lines go to run_out/ under the repository root.
set -e
TAG=${1:-r02}; shift || true
STEPS=${*:-tests bench prof}
OUT=run_out
mkdir -p $OUT
for s in $STEPS; do
  case $s in
    tests)
      timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/gputests_$TAG.log 2>&1 || { tail -40 $OUT/gputests_$TAG.log; exit 1; }
      tail -3 $OUT/gputests_$TAG.log ;;
    bench)
      timeout -k 10 500 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -30 $OUT/bench_$TAG.err; exit 1; }
      cat $OUT/bench_$TAG.json ;;
    prof)
      bash tools/profile_round.sh $TAG ;;
  esac
done
