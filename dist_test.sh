#!/usr/bin/env bash
# Multi-GPU evaluation: bash dist_test.sh CONFIG CHECKPOINT GPUS [test.py options]
# NNODES, NODE_RANK, PORT and MASTER_ADDR come from the environment (defaults: one node, rank 0, 29500, 127.0.0.1).
set -e
if [ "$#" -lt 3 ]; then
    echo "usage: $0 CONFIG CHECKPOINT GPUS [test.py options]" >&2
    exit 2
fi
CONFIG=$1
CHECKPOINT=$2
GPUS=$3
shift 3
HERE="$(cd "$(dirname "$0")" && pwd)"
export PYTHONPATH="$HERE${PYTHONPATH:+:$PYTHONPATH}"
python -m torch.distributed.run \
    --nnodes="${NNODES:-1}" \
    --node_rank="${NODE_RANK:-0}" \
    --master_addr="${MASTER_ADDR:-127.0.0.1}" \
    --nproc_per_node="$GPUS" \
    --master_port="${PORT:-29500}" \
    "$HERE/test.py" "$CONFIG" "$CHECKPOINT" --launcher pytorch "$@"
