#!/bin/bash
# sweep ring geometries of the fp8 C=128 tower (variant builds of the whole library, production flags); prints the tower's time
cd "$(dirname "$0")/../.."
for cfg in "6 3 3" "6 3 2" "3 3 3" "2 1 2" "4 2 2" "6 3 6" "12 9 3" "9 9 3"; do
  set -- $cfg
  python smart-chess-rust_amd/build.py --out smart-chess-rust_amd/lib_s --define SC_T8_RS=$1 --define SC_T8_TPI=$2 --define SC_T8_AB=$3 > /dev/null 2>&1 || { echo "RS=$1 TPI=$2 AB=$3 build failed"; continue; }
  echo "== RS=$1 TPI=$2 AB=$3"
  SC_PREC=fp8 SC_ENGINE_LIB=smart-chess-rust_amd/lib_s/libsc_engine.so timeout -k 10 300 python tools/tower_time.py 128 10 256 2>&1 | tail -1 || exit 1
done
