#!/bin/bash
# Diagnostic: build superdsm_amd/libsdsm_hip_<name>.so (or the product library for name = "main") with extra compiler flags, one object
# per source (objects of unchanged sources are reused: build/<name>/*.o).   usage: bash tools/build_variant.sh <name> [-DFOO=1 ...]
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
src=${SDSM_SRC:-$root/superdsm_amd/csrc}
out=$root/build/$name; mkdir -p "$out"
flags="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -munsafe-fp-atomics $*"
echo "$flags" > "$out/flags.new"
if ! cmp -s "$out/flags.new" "$out/flags" 2>/dev/null; then rm -f "$out"/*.o; mv "$out/flags.new" "$out/flags"; fi
pids=()
sources=$(cd "$root" && python3 -c "import __graft_entry__ as g; print(' '.join(g.SOURCES))")      # the product's own list
for f in $sources; do
  o=$out/${f%.*}.o
  stale=0                                        # every header is a dependency of every object
  for d in "$src/$f" "$src"/*.h "$root/include/sdsm.h"; do if [ ! -f "$o" ] || [ "$d" -nt "$o" ]; then stale=1; fi; done
  if [ $stale = 1 ]; then
    /opt/rocm/bin/hipcc $flags -c "$src/$f" -o "$o" & pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
lib=$root/superdsm_amd/libsdsm_hip_$name.so
[ "$name" = main ] && lib=$root/superdsm_amd/libsdsm_hip.so
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$lib" "$out"/*.o
echo "built $lib"
