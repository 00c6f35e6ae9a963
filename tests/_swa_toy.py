"""Small torch models for the stochastic-weight-averaging tests of the training loop: Linear-BN-ReLU-Linear, and
the same without the BatchNorm (the schedule differs: no re-estimate epoch)."""
import torch.nn as nn


class ToyBN(nn.Module):
    def __init__(self, num_classes: int = 5, in_samples: int = 16, hidden: int = 12):
        super().__init__()
        self.net = nn.Sequential(nn.Flatten(), nn.Linear(in_samples, hidden), nn.BatchNorm1d(hidden), nn.ReLU(),
                                 nn.Linear(hidden, num_classes))

    def forward(self, x):
        return self.net(x)


class ToyPlain(nn.Module):
    def __init__(self, num_classes: int = 5, in_samples: int = 16, hidden: int = 12):
        super().__init__()
        self.net = nn.Sequential(nn.Flatten(), nn.Linear(in_samples, hidden), nn.ReLU(),
                                 nn.Linear(hidden, num_classes))

    def forward(self, x):
        return self.net(x)
