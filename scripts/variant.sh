#!/bin/bash
# Build an A/B variant library ppo-bipedalwalker_amd/libwk_<name>.so that recompiles only the
# listed objects with extra flags and takes the rest from build/ (run `make` first):
#   bash scripts/variant.sh <name> "<flags>" <target> [<target> ...]
# A target is a source of csrc/ (wk_ppo_mfma.hip; a rollout unit such as wk_env_pair.hip) or
# wk_env for all eight rollout units.  The objects are rebuilt by the Makefile's own rules, so
# every one gets the flags it ships with (wk_env_quad.hip the default scheduler) plus <flags>:
# as PHYS_EXTRA when only rollout units are rebuilt, as EXTRA otherwise.
# PHYS_SCHED in the environment replaces the physics scheduler option.
set -eu
cd "$(dirname "$0")/../ppo-bipedalwalker_amd"
name=$1; flags=$2; shift 2
B=build_$name
rm -rf $B; mkdir -p $B; cp build/*.o $B/
var=PHYS_EXTRA
for t in "$@"; do
  case $t in
    wk_env) rm -f $B/wk_env*.hip.o;;
    *) [ -f csrc/$t ] || { echo "no source csrc/$t" >&2; exit 2; }
       rm -f $B/$t.o
       case $t in wk_env*.hip) ;; *) var=EXTRA;; esac;;
  esac
done
make -s -j"${JOBS:-8}" BUILD=$B LIB=libwk_$name.so "$var=$flags"
echo built libwk_$name.so
