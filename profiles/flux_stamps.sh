#!/bin/bash
# Developer aid (GPU box): per-phase cycle stamps of one workgroup of vag_flux_grid_kernel on the C2 bench batch
# (variants/libvag_stamps.so = profiles/build_variant.sh stamps -DVAG_FLUX_STAMPS), then the timing of every other variant.
cd "$(dirname "$0")/.."
# The headline batch takes the split form (vag_flux_grid_split_kernel): its lines are "split A wave" (cycles inside the boundary loop,
# passes, cycles of the item, cycles from barrier release to the first boundary item, and on the EAT wavefronts from the end of the
# boundary loop to the first log2_tab_core) and "split B wave" (cycles inside the interpolation, cycles from barrier release to the
# first bracket).  Both end in what the wavefront spends between the rows: "fill", the cycles from the head of the item loop (the
# claim) to the release of the barrier before the item's first row, and "restage C in N", the cycles from the N barrier releases that
# found another photon block to the release behind its staging and EAT step.  "item" counts from the claim.  VAG_FLUX_SPLIT=0 stamps
# the plain kernel.
VAG_LIB_PATH=$PWD/variants/libvag_stamps.so python bench.py --no-cpu-baseline --no-walkers --steps 1 --warmup 0 2>&1 | grep -E "flux wave|split [AB] wave" | head -16
for f in variants/libvag_*.so vegasafterglow_amd/libvegasafterglow_amd.so; do
  case $f in *stamps*) continue;; esac
  echo "== $f"
  VAG_LIB_PATH=$PWD/$f python bench.py --no-cpu-baseline --no-walkers --steps 4 --warmup 1 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(round(d['value']), d['stage_ms'])"
done
