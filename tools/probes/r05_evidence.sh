#!/bin/bash
# Round 5 evidence pass (one box): everything lands in gpurun_out/r05/, the files that are judged are then copied to profiles/.
#   gpurun -- 'DEFTET_COMMIT=<git rev-parse HEAD> tools/probes/r05_evidence.sh [part ...]'     parts: pmc bench prof ab stage tol (default: all)
cd "$GRAFT_REPO_ROOT"; export TMPDIR=/tmp
O=gpurun_out/r05; mkdir -p $O
parts="${*:-pmc bench prof ab stage tol}"
B="python $PWD/bench.py --full"      # (--full: the lines below quote the median step, hipGraph replay and the other configurations)
Q="--no-cpu-baseline --no-other-configs --no-bandwidth-probe --no-brute-force"
has() { case " $parts " in *" $1 "*) return 0;; esac; return 1; }

if has pmc; then
  PMC_TRAFFIC_OUT=$O/r05_pmc_traffic.json tools/pmc_run.sh $O/r05_pmc_traversal.json k_tet_scan -- $B --steps 5 --warmup 2 $Q
  PMC_PASSES="0 1 4 5" tools/pmc_run.sh $O/r05_pmc_raster.json k_pix_raster -- $B --config 4 --steps 3 --warmup 1 $Q
  PMC_PASSES="0 1" tools/pmc_run.sh $O/r05_pmc_geometry.json k_tri_query_coop -- $B --config 5 --steps 2 --warmup 1 $Q
  cp $O/r05_pmc_traffic.json $O/r05_pmc_raster.json $O/r05_pmc_geometry.json profiles/     # bench.py quotes traffic / VALU counts from profiles/
fi
if has bench; then
  $B 2> $O/bench_default.err | tail -1 > $O/r05_bench_line.json
  rm -f $O/r05_bench_line_driver_style.jsonl
  for i in 1 2 3; do $B --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs --no-brute-force 2>/dev/null | tail -1 >> $O/r05_bench_line_driver_style.jsonl; done
  DEFTET_BENCH_QUERY_BOX=measure $B --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs --no-brute-force 2>/dev/null | tail -1 > $O/r05_bench_line_measured_box.json
  rm -f $O/r05_bench_lines_raster_geometry.jsonl
  for c in 4 5; do $B --config $c --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs --no-bandwidth-probe 2>/dev/null | tail -1 >> $O/r05_bench_lines_raster_geometry.jsonl; done
fi
if has prof; then
  for spec in "2 r05_bench" "4 r05_raster_step" "5 r05_geometry_step"; do
    set -- $spec
    rm -rf $O/prof_$1
    (cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/$O/prof_$1 -o p -- $B --config $1 --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs --no-brute-force --no-bandwidth-probe 2>/dev/null | tail -1 > $GRAFT_REPO_ROOT/$O/$2_line_under_rocprof.json)
    f=$(find $O/prof_$1 -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $O/$2_kernel_stats.csv
    rm -rf $O/prof_$1
  done
fi
if has ab; then
  tools/probes/r05_orders_ab.sh > $O/orders_ab.txt 2>&1; cp gpurun_out/r05_scan_ab_orders.jsonl $O/
  rm -f $O/r05_scan_ab_kernels.jsonl
  for c in 2 3 1; do for a in 4 5 3; do python tools/probes/scan_variants.py --config $c --algo $a --tet-order native --reps 30 2>/dev/null >> $O/r05_scan_ab_kernels.jsonl; done; done
  rm -f $O/r05_step_kernels.jsonl
  for c in 2 1 3; do python tools/probes/sort_probe.py --config $c 2>/dev/null | tail -1 >> $O/r05_step_kernels.jsonl; done
  for c in 2 3; do DEFTET_HIP_LIB=$PWD/tools/probes/bin/libdeftet_phase.so python tools/probes/phase_probe.py --algo 4 --config $c 2>/dev/null | tail -2; done > $O/r05_phase_and_ungrouped_lanes.jsonl
fi
if has stage; then
  STAGES="1 2 3 4 5 0" tools/probes/r05_stage_insts.sh > $O/r05_stage_insts.txt 2>&1
  rm -f $O/r05_wave_spans.jsonl
  for c in 2 3; do DEFTET_HIP_LIB=$PWD/tools/probes/bin/libdeftet_phase.so python tools/probes/span_probe.py --config $c 2>/dev/null | tail -1 >> $O/r05_wave_spans.jsonl; done
  DEFTET_HIP_LIB=$PWD/tools/probes/bin/libdeftet_phase.so python tools/probes/occupancy_probe.py 2>/dev/null | tail -1 > $O/r05_occupancy.txt
fi
if has tol; then
  rm -f $O/r05_tolerances.jsonl
  DEFTET_TOLERANCE_REPORT=$PWD/$O/r05_tolerances.jsonl timeout 900 python -m pytest tests -m gpu -q > $O/pytest_gpu.log 2>&1
  grep -v amdgpu.ids $O/pytest_gpu.log | tail -3
fi
ls -la $O
