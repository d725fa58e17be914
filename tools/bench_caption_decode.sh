#!/bin/bash
# The caption token loop on native against e4m3 weights (tools/bench_caption_decode.py), as one GPU step under its own time limit.
#   tools/bench_caption_decode.sh [OUT]      default OUT: profiles/caption_e4m3_ab.txt
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/caption_e4m3_ab.txt}
timeout -k 10 900 python tools/bench_caption_decode.py --out "$OUT"
