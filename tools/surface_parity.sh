#!/bin/bash
# Byte parity of the C++ surface's tools (bin/enhance, bin/denoise) against another build of them, e.g. the parent commit's:
#   tools/surface_parity.sh <dir with the other build's enhance and denoise> <output dir>
# (the other build's binaries find their libnle_hip.so through their own rpath, ../lib beside them).  Every configuration
# runs on tests/golden/flower-50.bmp with 10 20 100 30 50 30 2 3 4 1 under both builds; the written files are compared
# with cmp, stdout, stderr and the exit codes with diff; then five plain runs each, alternating, for the wall time.
# One line per configuration and run goes to <output dir>/parity.txt.  Every GPU step has its own time limit, and an
# abort, a fault or a time-out ends the script there.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OLD=$(cd "$1" && pwd)
mkdir -p "$2"
OUT=$(cd "$2" && pwd)
NEW=$R/nonlocal-image-edit_amd/bin
LOG=$OUT/parity.txt
: > "$LOG"
SRC=$R/tests/golden/flower-50.bmp
CROP=$OUT/crop64x48.bmp
MASK=$OUT/mask_corner.bmp
ARGS="10 20 100 30 50 30 2 3 4 1"
# the exact filter's input (at most 64 x 64) and a stroke mask covering the top-left corner
python3 - "$SRC" "$CROP" "$MASK" <<'EOF' || exit 1
import sys
import numpy as np
from PIL import Image
im = Image.open(sys.argv[1]).convert("RGB")
im.crop((100, 60, 164, 108)).save(sys.argv[2])
m = np.zeros((im.size[1], im.size[0], 3), np.uint8)
m[:80, :100] = 255
Image.fromarray(m).save(sys.argv[3])
EOF

step() {  # step <seconds> <stdout file> <stderr file> command...
    local t=$1 so=$2 se=$3
    shift 3
    timeout -k 10 "$t" "$@" > "$so" 2> "$se"
    local rc=$?
    case $rc in
        124|137|134|135|136|139) echo "ENDED rc=$rc: $*" | tee -a "$LOG"; tail -5 "$se" | tee -a "$LOG"; exit $rc ;;
    esac
    if grep -qi "illegal memory access\|HSA_STATUS_ERROR" "$se" "$so"; then
        echo "GPU ERROR: $*" | tee -a "$LOG"; tail -5 "$se" | tee -a "$LOG"; exit 99
    fi
    return $rc
}

pair() {  # pair <tag> <tool> <input> <positional arguments> [leading options...]; PAIR_ENV: VAR=value for both runs
    local tag=$1 tool=$2 input=$3 targs=$4 res=identical side bin o
    shift 4
    for side in old new; do
        bin=$OLD
        [ $side = new ] && bin=$NEW
        local lead=()
        for o in "$@"; do lead+=("${o//@SIDE@/$side}"); done
        step 180 "$OUT/$tag.$side.stdout" "$OUT/$tag.$side.stderr" env ${PAIR_ENV:-} "$bin/$tool" "${lead[@]}" "$input" "$OUT/$tag.$side.bmp" $targs
        echo $? > "$OUT/$tag.$side.rc"
        sed -i "s#$bin/##" "$OUT/$tag.$side.stderr"  # argv[0] in the usage line
    done
    if [ -e "$OUT/$tag.old.bmp" ] || [ -e "$OUT/$tag.new.bmp" ]; then
        cmp -s "$OUT/$tag.old.bmp" "$OUT/$tag.new.bmp" || res="OUTPUT DIFFERS"
    else
        res="no file written by either"
    fi
    diff -q "$OUT/$tag.old.stdout" "$OUT/$tag.new.stdout" > /dev/null || res="$res, STDOUT DIFFERS"
    diff -q "$OUT/$tag.old.stderr" "$OUT/$tag.new.stderr" > /dev/null || res="$res, STDERR DIFFERS"
    cmp -s "$OUT/$tag.old.rc" "$OUT/$tag.new.rc" || res="$res, EXIT CODE DIFFERS"
    if [ -e "$OUT/$tag.old.map.bmp" ] || [ -e "$OUT/$tag.new.map.bmp" ]; then
        cmp -s "$OUT/$tag.old.map.bmp" "$OUT/$tag.new.map.bmp" && res="$res, map identical" || res="$res, MAP DIFFERS"
    fi
    echo "$tag: exit $(cat "$OUT/$tag.old.rc") / $(cat "$OUT/$tag.new.rc"), $(stat -c %s "$OUT/$tag.new.bmp" 2> /dev/null || echo 0) bytes, $(wc -l < "$OUT/$tag.new.stdout") stdout lines, $(wc -c < "$OUT/$tag.new.stderr") stderr bytes: $res" | tee -a "$LOG"
}

PAIR_ENV=
pair plain enhance "$SRC" "$ARGS"
pair patch_radius_1 enhance "$SRC" "$ARGS" --patch-radius 1
pair sampler_farthest enhance "$SRC" "$ARGS" --sampler farthest
pair sampler_residual enhance "$SRC" "$ARGS" --sampler residual
pair chroma_20 enhance "$SRC" "$ARGS" --chroma 20
pair region enhance "$SRC" "$ARGS" --region "$MASK:1,1,2,1"
pair nystrom_report enhance "$SRC" "$ARGS" --nystrom-report --nystrom-map "$OUT/nystrom_report.@SIDE@.map.bmp"
pair exact_crop enhance "$CROP" "$ARGS" --exact
pair denoise_7_numbers denoise "$SRC" "10 20 100 30 10 30 2"          # two short of denoise's argv: the usage line
pair denoise denoise "$SRC" "10 20 100 30 10 30 10 10 2"              # the same with sigma colour, sigma space = 10, 10
PAIR_ENV="NLE_DEVICES=0,0"
pair devices_0_0 enhance "$SRC" "$ARGS"
PAIR_ENV="NLE_DEVICES=0,0,0"
pair devices_0_0_0 enhance "$SRC" "$ARGS"
PAIR_ENV=

for i in 1 2 3 4 5; do  # wall time of the whole process, plain enhance
    for side in old new; do
        bin=$OLD
        [ $side = new ] && bin=$NEW
        t0=$(date +%s%N)
        step 180 "$OUT/time.stdout" "$OUT/time.stderr" "$bin/enhance" "$SRC" "$OUT/time.bmp" $ARGS || { echo "timing run failed" | tee -a "$LOG"; exit 1; }
        t1=$(date +%s%N)
        echo "time $side run $i: $(( (t1 - t0) / 1000000 )) ms" | tee -a "$LOG"
    done
done
for side in old new; do
    echo "time $side: min / median / max $(grep "^time $side run" "$LOG" | awk '{print $5}' | sort -n | awk '{v[NR]=$1} END {print v[1], "/", v[3], "/", v[5]}') ms" | tee -a "$LOG"
done
echo "parity done" | tee -a "$LOG"
