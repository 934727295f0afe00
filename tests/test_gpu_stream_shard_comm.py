"""The stream on two ranks as two processes sharing the GPU (DESIGN.md §3 rule 16), gloo as the host
transport, in the way tests/test_gpu_dist_host.py runs the batch exchange: rm_tilestore_exchange
through a communicator over host segments, and python -m reporter_amd.stream --ranks 2 --transport
host on the shared small stream, whose output directory must equal the one-rank run's in names and
bytes.  Every GPU step is a child process under its own time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_shard_ref as ss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_EXCHANGE_RANK = r"""
import json, os, sys
sys.path.insert(0, os.environ["RM_ROOT"])
sys.path.insert(0, os.path.join(os.environ["RM_ROOT"], "tests"))
import numpy as np
from reporter_amd import dist, engine
from test_gpu_stream_shard import _segments
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
comm = dist.GlooComm(rank, world, 0)
rng = np.random.default_rng(8)
segs = [_segments(rng, 900, 300), _segments(rng, 700, 300)]
cols = ("id", "next_id", "t0", "t1", "length", "queue_length")
store = engine.TileStore(0, 60, 2, initial_rows=4)
if rank == 0:      # rank 1 holds no row at the first exchange: the padded path
    store.add(*(segs[0][c] for c in cols))
else:
    store.add(*(np.zeros(0, np.float64) for _ in cols))
first = store.exchange(comm)
files0, _ = store.flush()
store.add(*(segs[rank][c] for c in cols))
second = store.exchange(comm)
files1, _ = store.flush()
ms = store.exchange_ms()
store.close()
comm.close()
with open(os.path.join(os.environ["RM_OUT"], "rank%d.json" % rank), "w") as f:
    json.dump({"stats": [first, second], "files": [{k: v.decode() for k, v in x.items()} for x in (files0, files1)], "ms": ms}, f)
"""


def _launch(code_or_module, args, env, tmp_path, n=2, limit=240):
    """n ranks as fresh child processes, each under its own time limit."""
    procs = []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), RM_RDZV_DIR=str(tmp_path), RM_RDZV_TOKEN="t%d" % os.getpid(),
                 RM_RDZV_NONCE="n%d" % os.getpid(), RM_COMM_TIMEOUT_S="120")
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable] + code_or_module + args, env=e,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate() for p in procs]
    for p, (o, err) in zip(procs, outs):
        assert p.returncode == 0, (p.returncode, o[-2000:], err[-3000:])
    return outs


def test_exchange_through_a_communicator(built_lib, tmp_path):
    import anonymiser_ref as ar
    from test_gpu_stream_shard import _segments
    env = dict(os.environ, RM_ROOT=ROOT, RM_OUT=str(tmp_path))
    _launch(["-c", _EXCHANGE_RANK], [], env, tmp_path)
    got = [json.load(open(str(tmp_path / ("rank%d.json" % r)))) for r in range(2)]
    rng = np.random.default_rng(8)
    segs = [_segments(rng, 900, 300), _segments(rng, 700, 300)]
    cols = ("id", "next_id", "t0", "t1", "length", "queue_length")
    tup = lambda s: list(zip(*(s[c].tolist() for c in cols)))
    model = ar.Anonymiser(60, 2)
    model.add(tup(segs[0]))
    assert model.held() > 1024
    want0 = model.flush()[0]
    # the second exchange: both ranks' call of equal number, index by index, rank 0 first on ties
    both = sorted([(j, r, s) for r in range(2) for j, s in enumerate(tup(segs[r]))], key=lambda x: (x[0], x[1]))
    model.add([s for _, _, s in both])
    want1 = model.flush()[0]
    for k, want in enumerate((want0, want1)):
        f0, f1 = got[0]["files"][k], got[1]["files"][k]
        assert f0 and f1 and not set(f0) & set(f1)
        assert {n: b.encode() for n, b in dict(f0, **f1).items()} == dict(want)
    assert got[1]["stats"][0]["before"] == 0 and got[1]["stats"][0]["received"] > 0
    assert got[0]["stats"][0]["sent"] == got[1]["stats"][0]["received"]
    print("exchange ms", got[0]["ms"], got[0]["stats"])


def test_stream_cli_on_two_ranks_writes_the_one_rank_directory(built_lib, small_world, tmp_path):
    sc = ss.scenario(small_world)
    src = tmp_path / "in"
    src.mkdir()
    (src / "a.txt").write_bytes(b"".join(sc["texts"]))
    conf = tmp_path / "conf.json"
    conf.write_text(json.dumps({"meili": {"default": {}}, "reporter_amd": {"graph": small_world}}))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), RM_RDZV_DIR=str(tmp_path),
               RM_COMM_TIMEOUT_S="120")

    def cli(out, *more):
        r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, "-m", "reporter_amd.stream", "--formatter", "@sv@,@0@2@3@1@4",
                            "--match-config", str(conf), "--output-location", str(out), "--privacy", str(ss.PRIVACY),
                            "--quantisation", str(ss.Q), "--flush-interval", "150", "--max-vehicles", str(sc["n_vehicles"]),
                            "--poll-bytes", "32768", "--report-dist", str(ss.PARAMS["dist"]), "--report-count", str(ss.PARAMS["count"]),
                            "--report-time", str(ss.PARAMS["time_s"]), str(src)] + list(more),
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        stats = json.loads(r.stdout.strip().splitlines()[-1])
        written = {}
        for root, _, fs in os.walk(out):
            for f in fs:
                p = os.path.join(root, f)
                written[os.path.relpath(p, out)] = open(p, "rb").read()
        return stats, written

    one_stats, one = cli(tmp_path / "one")
    two_stats, two = cli(tmp_path / "two", "--ranks", "2", "--transport", "host")
    assert one and two == one
    assert one_stats["flushes"] >= 3 and one_stats["polls"] >= 4 and one_stats["dropped"] > 0
    assert two_stats == one_stats
    r = subprocess.run([sys.executable, "-m", "reporter_amd.stream", "--formatter", "@sv@,@0@2@3@1@4", "--match-config", str(conf),
                        "--output-location", str(tmp_path / "x"), "--ranks", "2", "--checkpoint", str(tmp_path / "c"), str(src)],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 2 and "--checkpoint" in r.stderr
