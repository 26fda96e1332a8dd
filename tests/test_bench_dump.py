"""bench.py --dump-outputs: the arrays written for an output-for-output comparison of two builds, and the --steps bound (host only:
the timed path itself runs on the MI355X)."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_arrays(tmp_path):
    toks = [torch.tensor([[5, 6, 7], [8, 9, 10]], dtype=torch.int32), torch.tensor([[151643, 0, 1]], dtype=torch.int32)]
    counts = [torch.tensor([3, 3], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)]
    compared = [{"agreement_rate": 87.5, "char_edit_distance": 3, "word_edit_distance": 1, "differing_segments": []}]
    merged = ["ab [c|d]", "é"]
    bench.dump_outputs(str(tmp_path / "out"), list(zip(toks, counts)), compared, merged)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == {"tokens", "token_counts", "merged_text", "merged_len", "compare_versions"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["tokens"], [[5, 6, 7], [8, 9, 10], [151643, 0, 1]])
    np.testing.assert_array_equal(got["token_counts"], [3, 3, 2])
    np.testing.assert_array_equal(got["merged_len"], [8, 1])
    assert "".join(chr(int(c)) for c in got["merged_text"][0]) == "ab [c|d]"
    np.testing.assert_array_equal(got["merged_text"][1], [0xE9] + [-1] * 7)
    np.testing.assert_array_equal(got["compare_versions"], [[87.5, 3, 1]])


def test_dump_outputs_without_a_second_read(tmp_path):
    bench.dump_outputs(str(tmp_path), [(torch.zeros(2, 4, dtype=torch.int32), torch.full((2,), 4, dtype=torch.int32))], [], ["", ""])
    assert sorted(os.listdir(tmp_path)) == ["merged_len.npy", "merged_text.npy", "token_counts.npy", "tokens.npy"]
    assert np.load(tmp_path / "merged_text.npy").shape == (2, 1)


def test_steps_must_be_positive():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert proc.returncode == 2 and "--steps must be >= 1" in proc.stderr


def test_full_is_an_option_of_its_own():
    """--full (the legs beside the headline) parses, and --steps stays bounded with it."""
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "0"], capture_output=True, text=True)
    assert proc.returncode == 2 and "--steps must be >= 1" in proc.stderr
