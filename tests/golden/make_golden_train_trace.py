"""Golden launch traces of the training graph: g16_train_graph_trace.json.gz (CPU only, no library).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_trace.py

Every scene of tests/train_trace.py (SCENES) runs its training steps (TrainGraph.forward + backward +
refresh_packs) on CPU tensors behind the recorder and its normalised calls are written one compact
line each, in the format of g15_aggregator_trace.json.gz (JSON, gzip-compressed with a zero
timestamp).  The fixture pins the launch sequence of sailrecon_amd/train/model.py, train/engine.py,
runtime.py and models/aggregator.py as they were at the commit named in its header (PARENT): with
those four files put back as of that commit this script writes the same bytes, and two runs of it
always do (the trace holds names, offsets and content hashes, no address).
tests/test_train_graph_trace.py compares the present code against it call by call."""

from __future__ import annotations

import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (os.path.join(REPO, "self-supervise-sfm_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import train_trace  # noqa: E402

# the commit whose train/model.py, train/engine.py, runtime.py and models/aggregator.py recorded the fixture
PARENT = "6b313fb"
OUT = os.path.join(HERE, "g16_train_graph_trace.json.gz")


def main():
    header = dict(parent=PARENT, models=train_trace.MODELS, call="[name, args, kwargs]",
                  tensor="[base, storage_offset, shape, stride, dtype(, sha1[:12] of int32 contents)]")
    lines = ['{"header":' + json.dumps(header, separators=(",", ":"), sort_keys=True) + ',', '"scenes":{']
    names = sorted(train_trace.SCENES)
    for i, name in enumerate(names):
        calls = train_trace.run_scene(name)
        lines.append(json.dumps(name) + ":[")
        lines += [train_trace.dump_call(c) + ("," if j + 1 < len(calls) else "") for j, c in enumerate(calls)]
        lines.append("]" + ("," if i + 1 < len(names) else ""))
        print(f"{name}: {len(calls)} calls")
    lines.append("}}")
    with open(OUT, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write(("\n".join(lines) + "\n").encode())
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
