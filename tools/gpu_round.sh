#!/bin/bash
# The GPU sessions of a round, by name (run on the gpurun box: gpurun -- 'bash tools/gpu_round.sh NAME ...').
# Every step runs under its own time limit (tools/gpu_session.sh); an A/B bench line prints the stage times.
#   tests     all GPU tests, then smoke()
#   bench     the default bench line with its CPU baseline (bench.py --full; written to $BENCH_JSON, default bench.json)
#   profile   rocprofv3 kernel trace + PMC passes of the default bench (gpurun_out/prof; tools/prof_summary.py)
#   modes     profiles of the VDICompositor and merged-bricks modes (gpurun_out/prof_comp, prof_merged)
#   timeline  per-ray search timeline of the one-brick share (emulated rank 7 of 8)
#   composite VDICompositor workload statistics and bench lines
#   emu       emulated per-GPU shares of 2, 4 and 8 GPUs, every rank
#   super     super-tile sampling order A/B (N=1, 8- and 4-GPU shares) + the sampling kernel's FETCH_SIZE
#   calib     FETCH_SIZE calibration for scattered 32-B / 8-B reads (tools/fetch_calib.hip) + request-size split
#   knobs5    round batch and search oversubscription A/B (N=1; 8-GPU share)
#   mknobs    the same knobs in merged-bricks mode
#   regroup   tail regrouping: the search GPU tests, A/B regroup=0/1, per-ray timelines
#   ab2       the working tree's library against a `head` variant (tools/rev_variant.sh REV head)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
export TMPDIR=/tmp
mkdir -p gpurun_out/ab
ab() {   # tag, extra bench args
    local tag=$1; shift
    timeout -k 10 150 python bench.py --steps 10 --warmup 2 --no-cpu-baseline "$@" > gpurun_out/ab/$tag.json 2> gpurun_out/ab/$tag.err || { echo "$tag FAILED"; tail -3 gpurun_out/ab/$tag.err; return 1; }
    python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); s=d['config']['stage_ms']; print(sys.argv[2], 'ms/step %.2f render %.2f sample %.2f search %.2f composite %.2f' % (d['ms_per_step'], s['render'], s['render.sample_kernel'], s['render.search_kernel'], s['composite']))" gpurun_out/ab/$tag.json "$tag"
}
abv() {   # tag, library, extra bench args: ab of a variant library (tools/rev_variant.sh, tools/variant_build.sh)
    local tag=$1 lib=$2; shift 2
    INSITU_HIP_LIB=$lib ab "$tag" "$@"
}
pmc() {   # tag, counters, extra bench args: one rocprofv3 PMC pass over a short N=1 bench run -> gpurun_out/pmc/<tag>
    local tag=$1 ctr=$2; shift 2
    mkdir -p gpurun_out/pmc
    timeout -k 10 300 rocprofv3 --pmc $ctr --kernel-include-regex insitu -d gpurun_out/pmc/$tag -o $tag -f csv -- \
        python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --update-every 0 "$@" > gpurun_out/pmc/$tag.log 2>&1 || { echo "pmc $tag FAILED"; return 1; }
    python3 tools/pmc_kernel_sum.py gpurun_out/pmc/$tag "$tag"
}
W8="--emulate-world 8 --emulate-rank 7 --update-every 0"
W4="--emulate-world 4 --emulate-rank 3 --update-every 0"
for name in "$@"; do
    case $name in
    tests) tools/gpu_session.sh \
        "gputests|700|python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread" \
        "smoke|200|python -c 'import __graft_entry__ as g; g.smoke()'" || exit $? ;;
    bench) tools/gpu_session.sh "bench|300|python bench.py --full > ${BENCH_JSON:-bench.json}" || exit $? ;;
    profile) tools/gpu_session.sh \
        "prof|600|PROF_OUT=gpurun_out/prof BENCH_ARGS='--steps 2 --warmup 1 --no-cpu-baseline' tools/profile_round.sh" || exit $? ;;
    modes) tools/gpu_session.sh \
        "prof_comp|500|PROF_OUT=gpurun_out/prof_comp BENCH_ARGS='--steps 2 --warmup 1 --no-cpu-baseline --compositor vdi --update-every 0' tools/profile_round.sh" \
        "prof_merged|700|PROF_OUT=gpurun_out/prof_merged BENCH_ARGS='--steps 2 --warmup 1 --no-cpu-baseline --merge-bricks --update-every 0' tools/profile_round.sh" || exit $? ;;
    timeline) tools/gpu_session.sh \
        "rt_w8|200|python tools/ray_timing.py 8 7 > gpurun_out/rt_w8.json" || exit $? ;;
    composite) tools/gpu_session.sh "comp_stats|300|python tools/composite_stats.py > gpurun_out/composite_stats.json" || exit $?
        ab comp --compositor vdi --update-every 0 && ab merged --merge-bricks --update-every 0 && ab n1 --update-every 0 || exit 1 ;;
    emu)   # per-rank render times of the emulated 2-, 4- and 8-GPU strong-scaling shares (tools/emu_ranks.sh)
        for w in 2 4 8; do EMU_WORLD=$w RAY_RANK=-1 tools/emu_ranks.sh || exit 1; done ;;
    calib) # FETCH_SIZE of known byte counts (tools/fetch_calib.hip, built in-tree) and the read-request size
        # split of the same patterns and of the default bench's kernels
        C=gpurun_out/calib
        mkdir -p $C
        SPLIT="TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum"
        tools/gpu_session.sh \
        "calib_bytes|60|tools/fetch_calib > $C/bytes.json" \
        "calib_trace|90|timeout -s KILL 80 rocprofv3 --kernel-trace --stats -d $C/trace -o trace -f csv -- tools/fetch_calib" \
        "calib_fetch|90|timeout -s KILL 80 rocprofv3 --pmc FETCH_SIZE -d $C/fetch -o fetch -f csv -- tools/fetch_calib" \
        "calib_split|90|timeout -s KILL 80 rocprofv3 --pmc $SPLIT -d $C/split -o split -f csv -- tools/fetch_calib" \
        "bench_split|300|timeout -s KILL 280 rocprofv3 --pmc $SPLIT --kernel-include-regex insitu -d $C/bench_split -o bench_split -f csv -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline" || exit $? ;;
    super) # longest-first order by super-tiles of 1/2/4 tiles per edge: N=1, the 8- and 4-GPU shares, sampling FETCH
        for s in 1 2 4; do
            ab n1_s$s --option super_tile=$s --update-every 0 && ab w8_s$s --option super_tile=$s $W8 &&
                ab w4_s$s --option super_tile=$s $W4 || exit 1
        done
        for s in 1 4; do pmc fetch_s$s FETCH_SIZE --option super_tile=$s || exit 1; done ;;
    knobs5) # round batch and search oversubscription after the select-form replay (N=1; 8-GPU share)
        U="--update-every 0"
        for rep in a b; do
            ab kb28$rep $U && ab kb36$rep $U --option round_batch=36 && ab kb20$rep $U --option round_batch=20 &&
                ab ko8$rep $U --option search_oversub=8 || exit 1
        done
        ab w8_ko6 $W8 && ab w8_ko8 $W8 --option search_oversub=8 && ab w8_ko4 $W8 --option search_oversub=4 || exit 1 ;;
    ab2) # the working tree's library against HEAD's (variant head): N=1 twice, plain, the 8-GPU share
        H=scenery-insitu_amd/lib/variants/libinsitu_hip_head.so
        U="--update-every 0"
        ab x_new $U && abv x_head $H $U && ab x_new2 $U && abv x_head2 $H $U && ab xp_new --mode plain $U &&
            abv xp_head $H --mode plain $U && ab xw8_new $W8 && abv xw8_head $H $W8 || exit 1 ;;
    mknobs) # merged mode: round batch 20 / 36 and search oversubscription 4 / 8 against the defaults (28, 6)
        M="--merge-bricks --update-every 0"
        ab mk_def $M && ab mk_rb20 $M --option round_batch=20 && ab mk_rb36 $M --option round_batch=36 &&
            ab mk_os4 $M --option search_oversub=4 && ab mk_os8 $M --option search_oversub=8 && ab mk_def2 $M || exit 1 ;;
    regroup) # tail regrouping: the search GPU tests, A/B regroup=0/1 at N=1 and on the 8- and 4-GPU shares, timelines
        tools/gpu_session.sh "gt_search|600|python -u -m pytest tests/test_gpu_parity.py -m gpu -x -q --timeout 200 --timeout-method thread" || exit $?
        for r in 0 1; do
            ab n1_rg$r --option regroup=$r --update-every 0 && ab w8_rg$r --option regroup=$r $W8 && ab w4_rg$r --option regroup=$r $W4 || exit 1
        done
        ab n1_rg0b --option regroup=0 --update-every 0 && ab n1_rg1b --option regroup=1 --update-every 0 || exit 1
        mkdir -p gpurun_out/rt
        timeout -k 10 150 python tools/ray_timing.py 4 3 > gpurun_out/rt/w4r3_rg1.json &&
            timeout -k 10 150 python tools/ray_timing.py 8 7 > gpurun_out/rt/w8r7_rg1.json || exit 1 ;;
    *) echo "unknown session $name"; exit 2 ;;
    esac
done
