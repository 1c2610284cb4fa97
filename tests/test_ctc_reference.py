"""The float64 model of the CTC layer (tests/ctc_reference.py) against torch.nn.functional.ctc_loss (float64, CPU).

Losses to 1e-10 relative, dL/dz (the model's dL/dy through the softmax Jacobian, against torch's gradient with respect to the
LOGITS: its gradient with respect to log_probs is not the plain derivative) to 1e-10 absolute."""
import numpy as np
import pytest
import torch

from ctc_reference import ctc_sequence, softmax_jacobian


def _torch_ctc(z, labels):
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    T, C = z.shape
    lp = torch.log_softmax(zt, dim=-1).unsqueeze(1)
    loss = torch.nn.functional.ctc_loss(lp, torch.tensor([labels], dtype=torch.long).reshape(1, -1), torch.tensor([T]),
                                        torch.tensor([len(labels)]), blank=C - 1, reduction="none")
    if torch.isfinite(loss).all():
        loss.sum().backward()
        return float(loss.detach()[0]), zt.grad.numpy()
    return float(loss.detach()[0]), None


def _case(name):
    rng = np.random.RandomState(11)
    if name == "random":
        return rng.randn(12, 6) * 2.0, [0, 3, 3, 1]
    if name == "repeated_labels":
        return rng.randn(15, 5) * 1.5, [2, 2, 2, 0, 2, 2]
    if name == "no_labels":
        return rng.randn(7, 4), []
    if name == "exactly_feasible":              # U + repeats == len: one alignment
        return rng.randn(7, 5), [1, 1, 1, 3]
    if name == "infeasible":                    # U + repeats = 8 > len = 7
        return rng.randn(7, 5), [1, 1, 1, 1, 3]
    if name == "uniform_400":                   # the plain product of 400 posteriors of 1/184 is 0 in float64
        assert (1.0 / 184.0) ** 400 == 0.0
        return np.zeros((400, 184)), list(rng.randint(0, 183, 60))
    raise KeyError(name)


@pytest.mark.parametrize("name", ["random", "repeated_labels", "no_labels", "exactly_feasible", "uniform_400"])
def test_model_matches_torch(name):
    z, labels = _case(name)
    y = torch.softmax(torch.tensor(z, dtype=torch.float64), dim=-1).numpy()
    loss, dldy, ok = ctc_sequence(y, labels, np.float64)
    t_loss, t_grad = _torch_ctc(z, labels)
    assert ok and np.isfinite(t_loss)
    rel = abs(loss - t_loss) / abs(t_loss)
    dz = np.abs(softmax_jacobian(y, dldy) - t_grad).max()
    print("%s: loss %.15g torch %.15g rel %.3g, dL/dz max abs diff %.3g" % (name, loss, t_loss, rel, dz))
    assert rel <= 1e-10
    assert dz <= 1e-10


def test_infeasible_sequence():
    z, labels = _case("infeasible")
    y = torch.softmax(torch.tensor(z, dtype=torch.float64), dim=-1).numpy()
    loss, dldy, ok = ctc_sequence(y, labels, np.float64)
    t_loss, _ = _torch_ctc(z, labels)
    assert np.isinf(t_loss)
    assert not ok and loss == 0.0 and not dldy.any()


def test_empty_sequence_is_infeasible():
    loss, dldy, ok = ctc_sequence(np.zeros((0, 5)), [1], np.float64)
    assert not ok and loss == 0.0 and dldy.shape == (0, 5)


def test_float32_model_stays_finite_at_2000_steps():
    rng = np.random.RandomState(5)
    z = rng.randn(2000, 40)
    y = torch.softmax(torch.tensor(z, dtype=torch.float64), dim=-1).numpy()
    labels = list(rng.randint(0, 39, 300))
    l64, g64, ok64 = ctc_sequence(y, labels, np.float64)
    l32, g32, ok32 = ctc_sequence(y.astype(np.float32), labels, np.float32)
    assert ok64 and ok32 and np.isfinite(g32).all()
    assert abs(float(l32) - l64) / l64 < 1e-5
    assert np.abs(y * g32 - y * g64).max() < 1e-3
