"""Multi-GPU path on CPU: two ranks over gloo exercise the page sharding and the token-stream gather that bench.py
and the batch driver use over RCCL (same code, backend "nccl")."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from handwritten_ocr_amd import shard


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cpu_rank():
    """Called first in every rank these tests spawn: the ranks are CPU processes (gloo, scripted reads), but torch's
    dist.barrier() probes for an accelerator, which on a GPU host initialises the GPU runtime in each of them — eight ranks
    beside the test runner are more processes than one shared GPU may have open.  They are told there is none."""
    torch._C._get_accelerator = lambda: torch.device("cpu")
    torch.cuda.is_available = lambda: False


def _worker(rank, world, port, q):
    _cpu_rank()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    r, _, w = shard.init_from_env(device_backend=False)
    pages = [f"page{i:02d}" for i in range(7)]            # 7 pages over 2 ranks: ragged shards (4 and 3)
    mine = shard.shard(pages, r, w)
    reads = 3 * len(mine)
    toks = torch.arange(reads * 5, dtype=torch.int32).view(reads, 5) + 1000 * r
    counts = torch.full((reads,), 5, dtype=torch.int32)
    got = shard.gather_token_streams(toks, counts, dst=0)
    if r == 0:
        q.put([(t.tolist(), c.tolist()) for t, c in got])
    else:
        assert got is None
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert len(got) == 2
    (t0, c0), (t1, c1) = got
    assert len(t0) == 12 and len(t1) == 9                 # 4 pages x 3 reads, 3 pages x 3 reads
    assert t0[0] == [0, 1, 2, 3, 4] and t1[0] == [1000, 1001, 1002, 1003, 1004]
    assert c0 == [5] * 12 and c1 == [5] * 9


def test_shard_helpers_single_process():
    pages = list(range(10))
    parts = [shard.shard(pages, r, 4) for r in range(4)]
    assert sorted(sum(parts, [])) == pages and [len(p) for p in parts] == [3, 3, 2, 2]
    own = shard.owner_index(10, 4)
    for i, (r, j) in enumerate(own):
        assert parts[r][j] == i
    t = torch.zeros(2, 3, dtype=torch.int32)
    assert shard.gather_token_streams(t, torch.tensor([3, 3], dtype=torch.int32))[0][0] is t


# ---------------------------------------------------------------------------------------------------------------------------
# The batch-folder driver over 2 ranks (gloo): every rank reads its share with a scripted engine, rank 0 gathers the token
# streams and writes ALL pages' files; the files must equal those of the 1-rank run byte for byte.
def _scripted_tokens(images, params=None, on_done=None, long=False):
    """Deterministic 'reads': the text depends only on the pixels handed to the engine (so it is the same whichever rank
    reads the page), with lengths that differ per read (ragged gather).  Reads are reported (on_done) out of order, a few at a time
    with a pause between, as an engine's decode slots release them.  `long`: page-length texts (~1.5 k characters)."""
    import hashlib
    import time

    import numpy as np

    out = []
    for im in images:
        h = hashlib.sha1(np.asarray(im).tobytes()).hexdigest()
        words = [h[i: i + 4] for i in range(0, 4 * (3 + int(h[0], 16) % 5), 4)]
        if long:
            words = [h[(7 * i) % 36: (7 * i) % 36 + 2 + i % 5] for i in range(300)]
        out.append(list(" ".join(words).encode("utf-8")))
    if on_done is not None:
        order = sorted(range(len(out)), key=lambda i: (i // 7, -i))
        for n, i in enumerate(order):
            if n % 7 == 0:
                time.sleep(0.002)
            on_done(i, out[i])
    return out


def _folder_worker(rank, world, port, src, out_dir, q, long=False):
    _cpu_rank()
    import contextlib
    import functools
    import io

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from handwritten_ocr_amd import batch, tools

    shard.init_from_env(device_backend=False)
    tools.run_ocr_batch_tokens = functools.partial(_scripted_tokens, long=long)
    tools.decode_tokens = lambda streams: [bytes(t).decode("utf-8") for t in streams]
    stats = {}
    with contextlib.redirect_stdout(io.StringIO()):
        outs = batch.transcribe_folder(batch.list_images(src), out_dir, quiet=True, stats=stats)
    q.put((rank, ([o.name for o in outs], stats)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _run_folder(world, src, out_dir, long=False, with_stats=False):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_folder_worker, args=(r, world, port, str(src), str(out_dir), q, long)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    return got if with_stats else {r: names for r, (names, _) in got.items()}


def _same_files(a_dir, b_dir, n_files):
    import json

    files = sorted(os.listdir(a_dir))
    assert files == sorted(os.listdir(b_dir)) and len(files) == n_files
    for fn in files:
        a, b = (a_dir / fn).read_text(), (b_dir / fn).read_text()
        if fn.endswith("_trace.json"):  # timestamps differ between runs; everything else must not
            strip = lambda evs: [{k: v for k, v in e.items() if k not in ("timestamp", "elapsed_seconds")} for e in evs]  # noqa: E731
            assert strip(json.loads(a)) == strip(json.loads(b)), fn
        elif fn.endswith("_trace_summary.txt"):
            assert [l.split("] ", 1)[1] for l in a.splitlines()] == [l.split("] ", 1)[1] for l in b.splitlines()], fn
        else:
            assert a == b, fn


def test_two_rank_folder_equals_one_rank(tmp_path):
    import json

    from PIL import Image

    from handwritten_ocr_amd.synth import make_page

    src = tmp_path / "pages"
    src.mkdir()
    for i in range(5):  # 5 pages over 2 ranks: shards of 3 and 2
        Image.fromarray(make_page(i, 64, 80), "RGB").save(src / f"page{i:02d}.png")
    one = _run_folder(1, src, tmp_path / "out1")
    two = _run_folder(2, src, tmp_path / "out2")
    names = [f"page{i:02d}_transcription.txt" for i in range(5)]
    assert one[0] == names
    assert two[0] == names and two[1] == []          # rank 0 writes every page, rank 1 writes nothing
    _same_files(tmp_path / "out1", tmp_path / "out2", 20)


def test_eight_rank_folder_equals_one_rank_and_rank0_keeps_up(tmp_path):
    """BASELINE config 3's shape on the CPU: 8 ranks (gloo), 141 pages - ragged shards of 18 and 17 pages, two gather rounds per
    rank, the second one short or EMPTY on some ranks - with page-length texts.  Files == the 1-rank run's, byte for byte; and rank
    0's host work per page (detokenise + initial_ocr replay with the native compare / merge + four files) is reported and held to
    the budget of a full node: 8 GPUs x 15 pages/s leave rank 0 1 / 120 s = 8.3 ms per page."""
    from PIL import Image

    from handwritten_ocr_amd import batch
    from handwritten_ocr_amd.synth import make_page

    src = tmp_path / "pages"
    src.mkdir()
    n = 141
    assert (n + 7) // 8 > batch.GATHER_PAGES and n - 7 * ((n + 7) // 8) >= 0
    for i in range(n):
        Image.fromarray(make_page(i, 32, 40), "RGB").save(src / f"page{i:03d}.png")
    one = _run_folder(1, src, tmp_path / "out1", long=True, with_stats=True)
    eight = _run_folder(8, src, tmp_path / "out8", long=True, with_stats=True)
    names = [f"page{i:03d}_transcription.txt" for i in range(n)]
    assert one[0][0] == names and eight[0][0] == names
    assert all(eight[r][0] == [] for r in range(1, 8))
    _same_files(tmp_path / "out1", tmp_path / "out8", 4 * n)
    st = eight[0][1]
    assert st["pages"] == n and st["gather_rounds"] == 2
    per_page_ms = 1e3 * st["rank0_host_s"] / n
    print(f"rank 0 host work: {per_page_ms:.2f} ms per page over {n} pages (8 ranks; budget 8.3 ms)")
    assert per_page_ms < 8.3, f"rank 0 needs {per_page_ms:.1f} ms of host time per page: it cannot keep up with 8 GPUs at 15 pages/s"


def test_ragged_width_gather_single_process_shapes():
    """Widths differ between ranks (reads stop at different lengths): exercised for real in the folder test above; here the
    degenerate single-process contract."""
    t = torch.zeros(0, 1, dtype=torch.int32)
    got = shard.gather_token_streams(t, torch.zeros(0, dtype=torch.int32))
    assert got[0][0].shape == (0, 1)


# A rank whose reads raise must not leave the others waiting in the gather until the backend's timeout: every rank
# learns who failed (shard.failed_ranks, before the data collective) and every rank leaves with an error, promptly.
def _failing_folder_worker(rank, world, port, src, out_dir, q):
    _cpu_rank()
    import contextlib
    import io
    import time

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from handwritten_ocr_amd import batch, tools

    shard.init_from_env(device_backend=False)

    def reads(images, params=None, on_done=None):
        if rank == 1:
            raise ValueError("unreadable page on rank 1")
        return _scripted_tokens(images, params, on_done)

    tools.run_ocr_batch_tokens = reads
    tools.decode_tokens = lambda streams: [bytes(t).decode("utf-8") for t in streams]
    t0 = time.time()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            batch.transcribe_folder(batch.list_images(src), out_dir, quiet=True)
        q.put((rank, "no error", time.time() - t0))
    except Exception as e:  # noqa: BLE001
        q.put((rank, f"{type(e).__name__}: {e}", time.time() - t0))
    dist.destroy_process_group()


def test_a_failing_rank_stops_every_rank_with_an_error(tmp_path):
    from PIL import Image

    from handwritten_ocr_amd.synth import make_page

    src = tmp_path / "pages"
    src.mkdir()
    for i in range(4):
        Image.fromarray(make_page(i, 64, 80), "RGB").save(src / f"page{i:02d}.png")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_failing_folder_worker, args=(r, 2, port, str(src), str(tmp_path / "out"), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (msg, dt) for r, msg, dt in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(120)
    assert got[1][0] == "ValueError: unreadable page on rank 1"
    assert got[0][0].startswith("RuntimeError: rank(s) [1] failed"), got[0]
    assert max(dt for _, dt in got.values()) < 60
    assert not (tmp_path / "out").exists() or not os.listdir(tmp_path / "out")
