#!/bin/bash
# Build an A/B variant library ppo-bipedalwalker_amd/libwk_<name>.so that recompiles only the
# listed objects with extra flags and takes the rest from build/ (run `make` first):
#   bash scripts/variant.sh <name> "<flags>" <target> [<target> ...]
# A target is a source of csrc/ (wk_ppo_mfma.hip; wk_physics.hip: all eight parts) or the number
# of one physics part (WK_PHYS_PART, see wk_physics.hip).  The objects are rebuilt by the
# Makefile's own rules, so every one gets the flags it ships with (part 8 the default scheduler)
# plus <flags>: as EXTRA for a source, as PHYS_EXTRA when only physics objects are rebuilt.
# PHYS_SCHED in the environment replaces the physics scheduler option.
set -eu
cd "$(dirname "$0")/../ppo-bipedalwalker_amd"
name=$1; flags=$2; shift 2
B=build_$name
rm -rf $B; mkdir -p $B; cp build/*.o $B/
var=PHYS_EXTRA
for t in "$@"; do
  case $t in
    wk_physics.hip) rm -f $B/wk_physics.hip.p*.o;;
    [1-8]) rm -f $B/wk_physics.hip.p$t.o;;
    *) [ -f csrc/$t ] || { echo "no source csrc/$t" >&2; exit 2; }
       rm -f $B/$t.o; var=EXTRA;;
  esac
done
make -s -j"${JOBS:-8}" BUILD=$B LIB=libwk_$name.so "$var=$flags"
echo built libwk_$name.so
