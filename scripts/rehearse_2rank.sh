OUT=${OUT:-run_out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_destriper.py -x -v -m gpu --timeout 200 --timeout-method thread -k two_ranks > $OUT/pytest_2rank.log 2>&1 || exit $?
COMAP_DIST_BACKEND=gloo timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29611 bench.py --gpus 2 --steps 2 --warmup 1 --feeds 6 --full --no-cpu-baseline --c5-obs 2 > $OUT/bench_2rank.log 2>&1
