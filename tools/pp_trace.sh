#!/bin/bash
# builds a PP_TRACE copy of the library into /tmp and runs the timeline dump (GPU box)
set -e
cd $GRAFT_REPO_ROOT/e4t-diffusion_amd/csrc
mkdir -p /tmp/ppobj
. ./units.sh      # UNITS, UNIT_FLAGS
for f in $UNITS; do
  if [ $f = gemm ]; then hipcc $UNIT_FLAGS -DPP_TRACE $PPFLAGS -c $f.hip -o /tmp/ppobj/$f.o; else cp obj/$f.o /tmp/ppobj/$f.o; fi
done
cp ../e4t/libe4t_hip.so /tmp/libe4t_hip.so.bak
hipcc --offload-arch=gfx950 -shared -fPIC $(printf '/tmp/ppobj/%s.o ' $UNITS) -ldl -o ../e4t/libe4t_hip.so
python $GRAFT_REPO_ROOT/tools/pp_trace.py
cp /tmp/libe4t_hip.so.bak ../e4t/libe4t_hip.so
