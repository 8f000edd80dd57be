#!/bin/bash
# Quick GPU check of the batch path after a change: parity / async / dist / deep-net tests, the
# pipeline probe and one headline bench line with the resident pass (no side legs).  Logs go to $OUT.
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
T="timeout -k 10"
$T 300 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_async.py tests/test_gpu_dist.py tests/test_deep_nn.py -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > "$OUT/t.log" 2>&1 && tail -3 "$OUT/t.log" && \
$T 120 python tools/pipe_probe.py c3_qp22 > "$OUT/pp.log" 2>&1 && \
$T 300 python bench.py --full --no-cpu-baseline --no-pi --no-tz --no-mc > "$OUT/b.log" 2>&1 && \
grep -v amdgpu.ids "$OUT/pp.log" && python -c "
import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(round(d['value']/1e6,1),round(d['ms_per_step'],4),{k:round(v,3) for k,v in d['roofline']['batch_kernel_ms'].items()},round(d['resident']['ms_per_step'],4))" "$OUT/b.log"
