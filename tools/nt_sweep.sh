# development tool: rebuild libnsx.so with each cache-policy mask (-DNSX_NT, nsx_internal.hpp) and run a short bench; on the GPU box
#   bash tools/nt_sweep.sh OUTDIR     (build logs and bench lines, with the per-kernel pass, go to OUTDIR)
set -e
OUT=${1:?usage: tools/nt_sweep.sh OUTDIR}
mkdir -p $OUT
for NT in ${NT_LIST:-0 1 4 5}; do
  make -B device HIPFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wall -Wno-unused-parameter -DNSX_NT=$NT" > $OUT/nt_build_$NT.log 2>&1
  python bench.py --full --steps 6 --warmup 2 --spinup 5 --no-cpu --profile-steps 4 > $OUT/nt_$NT.json 2> $OUT/nt_$NT.err
  echo "NT=$NT done"
done
