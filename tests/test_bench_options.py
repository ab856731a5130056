"""bench.py's plain run, ``--full`` and ``--dump-outputs``: the options parse, a dumped array
is float64 and the same from call to call, and (GPU) a plain run times exactly ``--steps``
steps, leaves the host baseline out and writes the last step's outputs reproducibly."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_options_parse(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--workload", "c1-dropin", "--dump-outputs", "out")


def test_dump_array_whole_and_sampled(tmp_path, monkeypatch):
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    small[0, 1], small[1, 2], small[2, 3] = float("nan"), float("inf"), float("-inf")
    bench._dump_array(str(tmp_path / "s"), small, np.random.default_rng(0))
    got, mark = np.load(tmp_path / "s.npy"), np.load(tmp_path / "s_nonfinite.npy")
    assert got.dtype == np.float64 and mark.dtype == np.float32 and np.isfinite(got).all()
    want = np.zeros((3, 4), dtype=np.float32)
    want[0, 1], want[1, 2], want[2, 3] = 1, 2, 3
    assert np.array_equal(mark, want)
    assert np.array_equal(got, np.where(want == 0, np.arange(12.0).reshape(3, 4), 0.0))
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    big = torch.arange(2 * 9 * 11, dtype=torch.float64).reshape(2, 9, 11)
    big[:, 5, :] = float("nan")
    for name in ("a", "b"):
        bench._dump_array(str(tmp_path / name), big, np.random.default_rng(0), own_lo=4)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    ma, mb = np.load(tmp_path / "a_nonfinite.npy"), np.load(tmp_path / "b_nonfinite.npy")
    assert a.shape == ma.shape == (50,) and np.array_equal(a, b) and np.array_equal(ma, mb)
    assert np.isfinite(a).all() and 0 < (ma == 1).sum() < 50 and (a[ma == 1] == 0).all()
    vals = a[ma == 0].astype(np.int64)
    assert ((vals // 11) % 9 >= 4).all()            # dimension 1 from own_lo on
    assert len(np.unique(vals)) > 20                # positions spread over the array


@pytest.mark.gpu
def test_plain_run_steps_and_dump(tmp_path, monkeypatch, capsys):
    from factormodeling_amd import pipeline as PL
    calls = []
    real = PL.run_step

    def counted(sp, cfg, **kw):
        calls.append(kw.get("timers") is not None)
        return real(sp, cfg, **kw)

    monkeypatch.setattr(PL, "run_step", counted)
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: pytest.fail("a plain run timed the host baseline"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    lines = []
    for name in ("a", "b"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dates", "128",
                                          "--assets", "300", "--factors", "12", "--dump-outputs", str(tmp_path / name)])
        bench.main()
        lines.append(json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]))
    assert calls == [False, True, True, True] * 2   # one warm-up, three timed steps, per run
    for line in lines:
        assert line["steps"] == 3 and line["cpu_baseline"] is None and line["dtype"] == "f64"
        assert line["value"] == pytest.approx(128 * 300 * 12 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert {"weights.npy", "weights_nonfinite.npy", "kept.npy", "op_buffer_0.npy",
            "op_buffer_0_nonfinite.npy"} <= set(files)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == (np.float32 if f.endswith("_nonfinite.npy") else np.float64), f
        assert np.isfinite(a).all() and np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 << 20
    w = np.load(tmp_path / "a" / "weights.npy")
    assert w.shape == (128 - 60 - 1, 12) and (w != 0).any()
    assert not np.load(tmp_path / "a" / "weights_nonfinite.npy").any()
    v, m = np.load(tmp_path / "a" / "op_buffer_0.npy"), np.load(tmp_path / "a" / "op_buffer_0_nonfinite.npy")
    assert v.shape == m.shape and (m == 0).any() and (v[m == 0] != 0).any() and (v[m != 0] == 0).all()
