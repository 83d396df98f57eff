#!/bin/bash
# builds /tmp/plan_bench (host planner timing, no GPU): bash tools/planbench/build.sh
R=$(cd $(dirname $0)/../.. && pwd)
# the csrc objects of build.SOURCES, by name (a glob over lib/obj would also link the object of a source that is gone)
OBJS=$(python -c "
import os, sys
sys.path.insert(0, '$R')
from tantivy_amd import build as B
B.build()
print(' '.join(os.path.join(B.OBJ_DIR, os.path.basename(s) + '.o') for s in B.SOURCES if os.sep + 'csrc' + os.sep in s))" 2>/dev/null | tail -1)
/opt/rocm/bin/hipcc -O3 -std=c++17 -Wno-unused-function -c $R/tools/planbench/plan_bench.cpp -o /tmp/plan_bench.o 2>/dev/null && \
/opt/rocm/bin/hipcc --offload-arch=gfx950 -o /tmp/plan_bench /tmp/plan_bench.o $OBJS -ldl -lpthread
