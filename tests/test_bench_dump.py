"""bench.py --dump-outputs (no GPU needed): the arrays are written as float32 .npy files, and an
array that would take the total past the size limit is written as a fixed, seeded sample."""
import numpy as np
import torch

import bench


def _outputs(B=3, T=5, U=4):
    g = torch.Generator().manual_seed(1)
    out = {"loss": torch.rand(B, generator=g), "grad": torch.rand((B, T, U, 2), generator=g)}
    return out, out["loss"].sum().reshape(1)


def test_dump_outputs_writes_every_array_whole(tmp_path):
    out, loss_sum = _outputs()
    bench.dump_outputs(tmp_path / "d", out, loss_sum)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["grad.npy", "loss.npy", "loss_sum.npy"]
    for name, want in (("loss", out["loss"]), ("grad", out["grad"]), ("loss_sum", loss_sum)):
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy())


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    out, loss_sum = _outputs()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256)  # grad alone is 480 B
    bench.dump_outputs(tmp_path / "a", out, loss_sum)
    bench.dump_outputs(tmp_path / "b", out, loss_sum)
    files = sorted((tmp_path / "a").iterdir())
    assert sum(p.stat().st_size - 128 for p in files) <= 256  # payload without the .npy headers
    idx = np.load(tmp_path / "a" / "grad_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "grad_index.npy"))
    assert len(np.unique(idx)) == len(idx) == (256 - 4 - 12) // 12
    got = np.load(tmp_path / "a" / "grad.npy")
    assert np.array_equal(got, out["grad"].numpy().reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "loss.npy"), out["loss"].numpy())
