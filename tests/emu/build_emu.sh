#!/bin/bash
# TEST INFRASTRUCTURE: build the host fiber-emulator flavour of the kernels (no GPU needed).  The same four translation
# units as the HIP build, compiled as C++ in parallel; the emulator runtime (GT_EMU_IMPL) lives in the first one.
# Several tests build the same variant library (libgroove_emu_big.so: tests/test_emu_kernels.py, tests/test_bf16_ops.py) and a suite
# split over processes runs them at the same time, so a build shares no file with another one: its objects live in a directory of its
# own and the library appears under its name by one rename.  (Shared objects once let a link read an object another build had just
# truncated -- the linker takes an empty file for an empty script -- and the library then loaded with a launcher undefined; a rename
# also leaves a process that has the previous library mapped with the file it opened.)
set -e
here="$(cd "$(dirname "$0")" && pwd)"
root="$(cd "$here/../.." && pwd)"
src="$root/transformergrooveinfilling_amd/csrc"
outlib="${GT_EMU_OUT:-$here/libgroove_emu.so}"
obj="$(mktemp -d "$here/obj_$(basename "$outlib" .so).XXXXXX")"
trap 'rm -rf "$obj"' EXIT
flags="-O2 -g -std=c++17 -DGT_EMU -x c++ -I$here -fPIC -Wall -Wno-unused-function -Wno-unused-variable -Wno-unknown-pragmas -Wno-unused-but-set-variable -Wno-psabi"
pids=()
g++ $flags -DGT_EMU_IMPL -c "$src/groove_hip.hip" -o "$obj/groove_hip.o" "$@" & pids+=($!)
g++ $flags -c "$src/groove_seq_fwd.hip" -o "$obj/groove_seq_fwd.o" "$@" & pids+=($!)
g++ $flags -c "$src/groove_seq_bwd.hip" -o "$obj/groove_seq_bwd.o" "$@" & pids+=($!)
g++ $flags -c "$src/groove_seq64.hip" -o "$obj/groove_seq64.o" "$@" & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
# (the temporary library keeps the .so suffix the ignore rules know, and sits beside its target: the rename stays on one file system)
g++ -shared -fPIC "$obj"/groove_hip.o "$obj"/groove_seq_fwd.o "$obj"/groove_seq_bwd.o "$obj"/groove_seq64.o -o "$obj/lib.so"
mv -f "$obj/lib.so" "$outlib"
echo "built $outlib"
