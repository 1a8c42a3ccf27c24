"""Helpers of the resumable-fit tests (test_resume_cpu.py, test_gpu_resume.py, gpu_resume_child.py):
a data generator that dies at a chosen batch of a chosen epoch, and the rows of a metrics.csv."""

import csv
import os


class InjectedCrash(RuntimeError):
    """What CrashAt raises: stands for the process dying in the middle of an epoch."""


class CrashAt(object):
    """Wraps a data generator; the ``batch``-th ``next_batch('train')`` call (0-based) of epoch
    ``epoch`` -- counted by the ``reset_iterators('train')`` calls -- raises InjectedCrash.
    ``epoch=None``: never (the unbroken run goes through the same wrapper)."""

    def __init__(self, gen, epoch=None, batch=0):
        self._gen, self._crash = gen, (epoch, batch)
        self._epoch, self._batch = -1, 0
        self.n_datasets = gen.n_datasets
        self.n_tot_batches = gen.n_tot_batches

    def __getattr__(self, name):
        return getattr(self._gen, name)

    def reset_iterators(self, dtype):
        if dtype in ('train', 'all'):
            self._epoch += 1
            self._batch = 0
        return self._gen.reset_iterators(dtype)

    def next_batch(self, dtype, **kw):
        if dtype == 'train':
            if (self._epoch, self._batch) == self._crash:
                raise InjectedCrash('injected crash at epoch %d, batch %d' % self._crash)
            self._batch += 1
        return self._gen.next_batch(dtype, **kw)


def read_rows(version_dir):
    """metrics.csv as a list of dicts (strings), without the wall-clock ``created_at``."""
    with open(os.path.join(version_dir, 'metrics.csv'), newline='') as f:
        rows = list(csv.DictReader(f))
    for row in rows:
        row.pop('created_at', None)
    return rows
