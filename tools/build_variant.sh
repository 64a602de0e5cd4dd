#!/bin/bash
# Build a variant of the HIP library for A/B runs (tools/ab.py, tools/pmc_ab.sh):
#   tools/build_variant.sh NAME [-DHUTK_...=..] ...   ->  hutoken_amd/lib/ab/NAME.so
# Sources and flags are hutoken_amd/build.py:build_hip's plus the given ones (the switches: hutoken_amd/csrc/hutk_lab.h).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
# (build.py loaded by path: importing the package would load, and perhaps build, the shipped library)
python3 -c '
import importlib.util, sys
spec = importlib.util.spec_from_file_location("hutk_build", sys.argv[1] + "/hutoken_amd/build.py")
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)
build.build_hip(force=True, extra_flags=sys.argv[3:], out=sys.argv[1] + "/hutoken_amd/lib/ab/" + sys.argv[2] + ".so")
' "$ROOT" "$NAME" "$@"
echo "built hutoken_amd/lib/ab/$NAME.so"
