"""CPU model of the batch filter's direct schedule (scripts/i8_batch_survival.py --direct): a
threshold from the exact keys of the sample rows the int8 ranking picks subtracts no bound width,
so at 20,000 x 768 it passes no more candidates than the certified bound of the same sample for
the same launch cuts.  No GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_thresholds_pass_no_more_candidates(capsys):
    spec = importlib.util.spec_from_file_location("i8_batch_survival",
                                                  os.path.join(ROOT, "scripts", "i8_batch_survival.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(["--rows", "20000", "--full", "20000", "--queries", "64", "--direct"])
    print(capsys.readouterr().out)
    five = (32, 96, 256, 512)
    for cuts in (five, ()):
        assert out["exact keys", cuts] <= out["bf16 bound", cuts], (cuts, out)
        assert out["exact keys, 2K rows", cuts] <= out["bf16 bound", cuts], (cuts, out)
    assert out["exact keys", five] <= out["exact keys", ()]   # the tighten passes only ever raise T
