"""Host side of the marginal-likelihood extension: the CLI argument and the header
declarations (tests/test_abi.py then checks binding and linkage of whatever the header
declares)."""
import os
import re

from vaeb_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_args_carries_iw_samples(capsys):
    assert cli.parse_args([])['iw_samples'] == 0
    a = cli.parse_args(['--iw_samples', '50', '--n_epochs', '1'])
    assert a['iw_samples'] == 50 and isinstance(a['iw_samples'], int)
    assert 'unused' not in capsys.readouterr().out


def test_argument_listing_is_unchanged_when_off(capsys):
    """Without --iw_samples the `Parameters used` listing is the one from before the argument
    existed; with it the value is listed like any other."""
    cli.print_args(cli.parse_args([]))
    off = capsys.readouterr().out
    assert 'iw_samples' not in off
    assert off.count('\n') == 3 + len(cli.command_line_args) + len(cli.command_line_flags)
    cli.print_args(cli.parse_args(['--iw_samples', '20']))
    assert '\tiw_samples: 20\n' in capsys.readouterr().out


class FakeModel:
    """Host-only stand-in with the VAEB attributes train_model uses."""
    calls = []

    def __init__(self, x_train, *a, **kw):
        self.N = x_train.shape[0]
        self.batch_size = 100
        self.objective = "sum_prior"

    def update_epoch(self, order):
        return -10.0 * len(order)

    def set_validation_data(self, x):
        self.nvalid = x.shape[0]

    def validate_resident(self):
        return -5.0 * self.nvalid

    def marginal_likelihood_resident(self, n_samples=50):
        FakeModel.calls.append(n_samples)
        return -4.0 * self.nvalid


def test_train_model_prints_the_line_only_when_asked(tmp_path, monkeypatch, capsys):
    from vaeb_amd import model
    monkeypatch.setattr(model, "VAEB", FakeModel)
    monkeypatch.chdir(tmp_path)
    FakeModel.calls.clear()
    cli.train_model(cli.parse_args(['--n_epochs', '2', '--synthetic', '--continuous']))
    off = capsys.readouterr().out
    assert 'Marginal' not in off and FakeModel.calls == []
    cli.train_model(cli.parse_args(['--n_epochs', '2', '--synthetic', '--continuous', '--iw_samples', '20']))
    on = capsys.readouterr().out.splitlines()
    assert FakeModel.calls == [20]   # once, after the last epoch
    assert on[-1] == "          [Marginal log-likelihood on validation set (K=20): -4.0]"
    assert on[-2] == "          [Lower bound on validation set: -5.0]"


def test_header_declares_the_three_functions():
    src = open(os.path.join(ROOT, "include", "vaeb_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for fn, args in (("vaeb_encode", 5), ("vaeb_marginal_ll", 6), ("vaeb_marginal_ll_resident", 3)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % fn, src)
        assert m, fn
        assert len(m.group(1).split(",")) == args, fn
