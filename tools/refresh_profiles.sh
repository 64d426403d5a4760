#!/bin/bash
# Run on the GPU box (gpurun): regenerates everything under profiles/ for the current code -> gpurun_out/refresh/
#   tools/refresh_profiles.sh [round-tag, default r02]
# Kernel traces and PMC passes are separate rocprofv3 runs (the pool refuses --pmc together with sys/hip traces);
# the program after `--` is python3 itself (no wrapper that re-execs).
set -x
export TMPDIR=/tmp
R=${1:-r06}
O=gpurun_out/refresh; mkdir -p $O
python bench.py --full --steps 20 --warmup 5 > $O/${R}_bench_config2_lm.json 2> $O/bench_config2_lm.err
python bench.py --full --solver trf --steps 5 --warmup 1 --no-cpu-baseline --no-parity-solver > $O/${R}_bench_config2_trf.json 2>> $O/bench.err
python bench.py --full --config 1 --no-cpu-baseline > $O/${R}_bench_config1_lm.json 2>> $O/bench.err
python bench.py --full --config 4 --no-cpu-baseline > $O/${R}_bench_config4_calib_lm.json 2>> $O/bench.err
python bench.py --full --config 3 --no-cpu-baseline --no-parity-solver > $O/${R}_bench_config3_one_gpu_lm.json 2>> $O/bench.err
# the opt_calib residual+Jacobian kernel (524 B/obs) at a size where a launch is not latency: configs[4]'s 7 cameras with 2M detections (1 GiB per launch)
python bench.py --full --config 4 --obs 2000000 --steps 3 --warmup 1 --no-cpu-baseline --no-parity-solver > $O/${R}_bench_config4_calib_2M_obs.json 2>> $O/bench.err
rocprofv3 --kernel-trace --stats -d $O/stats_lm -o r -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-parity-solver > $O/stats_lm.log 2>&1
python3 tools/rocprof_summary.py stats $O/stats_lm/r_results.db > $O/${R}_kernel_stats_config2_lm.txt
rocprofv3 --kernel-trace --stats -d $O/stats_trf -o r -- python3 bench.py --full --solver trf --steps 5 --warmup 1 --no-cpu-baseline --no-parity-solver > $O/stats_trf.log 2>&1
python3 tools/rocprof_summary.py stats $O/stats_trf/r_results.db > $O/${R}_kernel_stats_config2_trf.txt
rocprofv3 --kernel-trace --stats -d $O/stats_c3 -o r -- python3 bench.py --full --config 3 --no-cpu-baseline --no-parity-solver > $O/stats_c3.log 2>&1
python3 tools/rocprof_summary.py stats $O/stats_c3/r_results.db > $O/${R}_kernel_stats_config3_one_gpu_lm.txt
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pmc_fetch -o r -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-parity-solver > $O/pmc_fetch.log 2>&1
python3 tools/rocprof_summary.py pmc $O/pmc_fetch/r_results.db > $O/${R}_pmc_FETCH_SIZE_config2.txt
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pmc_write -o r -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-parity-solver > $O/pmc_write.log 2>&1
python3 tools/rocprof_summary.py pmc $O/pmc_write/r_results.db > $O/${R}_pmc_WRITE_SIZE_config2.txt
python3 tools/rocprof_summary.py traffic $O/${R}_pmc_FETCH_SIZE_config2.txt $O/${R}_pmc_WRITE_SIZE_config2.txt config2_calib0 > $O/pmc_traffic_c2.json
# configs[3] on one GPU (779 MB per launch of the judged kernel) and configs[4] (opt_calib: k_observations<true,true>)
for C in 3 4; do
  rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pmc_fetch$C -o r -- python3 bench.py --full --config $C --steps 3 --warmup 1 --no-cpu-baseline --no-parity-solver > $O/pmc_fetch$C.log 2>&1
  python3 tools/rocprof_summary.py pmc $O/pmc_fetch$C/r_results.db > $O/${R}_pmc_FETCH_SIZE_config$C.txt
  rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pmc_write$C -o r -- python3 bench.py --full --config $C --steps 3 --warmup 1 --no-cpu-baseline --no-parity-solver > $O/pmc_write$C.log 2>&1
  python3 tools/rocprof_summary.py pmc $O/pmc_write$C/r_results.db > $O/${R}_pmc_WRITE_SIZE_config$C.txt
done
python3 tools/rocprof_summary.py traffic $O/${R}_pmc_FETCH_SIZE_config3.txt $O/${R}_pmc_WRITE_SIZE_config3.txt config3_calib0 $O/pmc_traffic_c2.json > $O/pmc_traffic_c23.json
python3 tools/rocprof_summary.py traffic $O/${R}_pmc_FETCH_SIZE_config4.txt $O/${R}_pmc_WRITE_SIZE_config4.txt config4_calib1 $O/pmc_traffic_c23.json > $O/pmc_traffic.json
# the bare store stream the judged kernel is compared with, built on the box
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -o /tmp/store_bw tools/micro/store_bw.hip && /tmp/store_bw > $O/${R}_store_bw.txt 2>&1
bash tools/step_timeline.sh 2 > $O/${R}_step_timeline_config2.txt 2>&1
python3 tools/incremental_loop.py --solver trf --cpu-sample 2>&1 | grep -v "^Number\|^Doing\|^$" > $O/${R}_incremental_loop_trf.txt
python3 tools/incremental_loop.py --solver lm 2>&1 | grep -v "^Number\|^Doing\|^$" > $O/${R}_incremental_loop_lm.txt
python3 tools/xlevel_table.py > $O/${R}_xlevel_parity.txt 2>&1
python3 tools/time_neighbours.py > $O/${R}_neighbour_steps.txt 2>&1
# round 4: the window-major assembly against the detection-major one, per configuration and window length; its SQ counters; cycle probes
python3 tools/micro/check_win_assembly.py 2>&1 | grep -v amdgpu > $O/${R}_window_assembly_check.txt
MVUS_WIN_LIST=0,3,4,6,8,10,12,16,20 python3 tools/micro/time_win.py 2 1 3 4 2>&1 | grep -v amdgpu > $O/${R}_window_length_sweep.txt
bash tools/micro/pmc_win.sh 2 > $O/${R}_window_assembly_sq_counters_config2.txt 2>&1
python3 tools/micro/collective_latency.py 1 2>&1 | grep -v "amdgpu\|socket.cpp\|^RCCL\|^HIP\|^ROCm\|^Hostname\|^Librccl" > $O/${R}_collective_latency_world1.txt
python3 tools/micro/time_scene_ba.py > $O/${R}_scene_ba_default_config1.txt 2>&1
# the Schur product's counters (MFMA busy, L2 hits, HBM fetch), the 16x16 pivot chain in isolation, the loop with the oracle's clock on
# every BA (down-scaled flight; at the loop's 1e2 and at configs[1]'s 1e4), the loop at 1e4 at full size
bash tools/micro/pmc_gemm.sh 2 > $O/${R}_schur_gemm_counters_config2.txt 2>&1
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -o /tmp/ldl16_bench tools/micro/ldl16_bench.hip 2>/dev/null && /tmp/ldl16_bench > $O/${R}_ldl16_pivot_chain.txt 2>&1
python3 tools/incremental_loop.py --solver trf --obs 20000 --cpu-all 2>&1 | grep -v "^Number\|^Doing\|^$\|amdgpu" > $O/${R}_loop_oracle_clock_every_ba.txt
python3 tools/incremental_loop.py --solver trf --obs 20000 --cpu-all --motion-weights 1e4 2>&1 | grep -v "^Number\|^Doing\|^$\|amdgpu" > $O/${R}_loop_oracle_clock_every_ba_mw1e4.txt
for seed in 1 2 3; do echo "== seed $seed trf motion_weights 1e4"; python3 tools/incremental_loop.py --solver trf --motion-weights 1e4 --seed $seed 2>&1 | grep -v "^Number\|^Doing\|^$\|amdgpu" | tail -9; done > $O/${R}_loop_motion_weights_1e4.txt 2>&1
# round 5/6: fp64 vector / matrix issue and co-issue (aggregate per SIMD), the reduced solve per configuration (step timeline at configs[1] and [3]), A/B of the two reduced solvers
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -o /tmp/fp64_coissue tools/micro/fp64_coissue.hip 2>/dev/null && /tmp/fp64_coissue > $O/${R}_fp64_coissue.txt 2>&1
bash tools/step_timeline.sh 3 > $O/${R}_step_timeline_config3.txt 2>&1
bash tools/step_timeline.sh 1 > $O/${R}_step_timeline_config1.txt 2>&1
for c in 1 2 3 4; do for m in ldl gj; do echo "configs[$c] MVUS_RCS=$m: $(MVUS_RCS=$m python3 tools/step_breakdown.py $c 2>&1 | tail -1)"; done; done 2>/dev/null | grep "^configs" > $O/${R}_reduced_solver_ab.txt
rm -rf $O/stats_lm $O/stats_trf $O/stats_c3 $O/pmc_fetch* $O/pmc_write* $O/pmc_traffic_c2.json $O/pmc_traffic_c23.json
ls -la $O
# round 5: the band solver's one-rank path against its parts switched off (same box, three repetitions, ms per step: python wall / C++ solve)
bash tools/band_solver_ab.sh > $O/${R}_band_solver_ab.txt 2>/dev/null
# round 6: the default solver on BASELINE configs[4] (opt_calib + rs_bounds + KE: the bounded TRF), the LM driver with and without the
# speculative linearisation / carry-over (python wall, C++ wall, long solve), LM at configs[4] with the sequential driver for reference
python bench.py --full --config 4 --solver trf --steps 3 --warmup 1 --no-cpu-baseline --no-parity-solver > $O/${R}_bench_config4_calib_trf.json 2>> $O/bench.err
( python3 tools/micro/host_probe.py; echo "--- MVUS_NO_SPEC=1 MVUS_LM_NO_CARRY=1 (the sequential driver of rounds 2-5)"; MVUS_NO_SPEC=1 MVUS_LM_NO_CARRY=1 python3 tools/micro/host_probe.py ) 2>&1 | grep -v amdgpu > $O/${R}_lm_driver_spec_ab.txt
# round 6: one rank of an 8-rank time-sharded run, alone on the GPU (per-kernel times behind the multi-GPU model of DESIGN section 6);
# (window length, camera groups) sweep of the window-major assembly
bash tools/micro/shard_rank_probe.sh 2>&1 | grep -v amdgpu > $O/${R}_shard_rank_probe_world8.txt
{ echo; echo "== one iteration of the rank in launch order: configs[3] cut over 8, rank 3 (the last fill is the probe's rejected trial, not part of an accepted iteration)"; bash tools/micro/shard_rank_timeline.sh 3 1;
  echo; echo "== the same for the weak-scaled default"; bash tools/micro/shard_rank_timeline.sh 2 8; } 2>&1 | grep -v amdgpu >> $O/${R}_shard_rank_probe_world8.txt
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -w -o /tmp/fp64_clock tools/micro/fp64_clock.hip 2>/dev/null && /tmp/fp64_clock > $O/${R}_fp64_clock.txt 2>&1
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -w -o /tmp/bcr_rhs_probe tools/micro/bcr_rhs_probe.hip 2>/dev/null && /tmp/bcr_rhs_probe > $O/${R}_bcr_rhs_probe.txt 2>&1
bash tools/micro/win_group_sweep.sh 2>&1 | grep -v amdgpu > $O/${R}_window_groups_sweep.txt
