"""Writes tests/golden/ref/stagewise_decisions.json: what the REFERENCE's stage-wise book-keeping decides on made-up score
sequences.  Build container only (the reference tree is not on the GPU box; the fixture is).

    python tests/golden/make_stagewise_fixture.py [REFERENCE_ROOT]        (default: $MVIN_REFERENCE or /root/reference)

It imports the reference's train_util at run time and drives its two Train_info_record_* classes through the loop of
main.py:24-45 (stage 0, then up to five restarts, `if trn_info.sw_early_stop >= 3: break`), feeding per-epoch (eval, test)
scores through its own Eval_score_info.  Recorded per stage: max_eval / max_test after the stage's epochs, sw_early_stop after
train_over, and the stored best (eval, test) pair; per case: how many stages the loop ran.  The fixture holds recorded results
only -- nothing of the reference's source."""
import importlib
import io
import json
import logging
import os
import sys
import tempfile
from contextlib import redirect_stdout
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref", "stagewise_decisions.json")
H_HOP = 2

# stage -> epochs of (eval, test); the value is eval AUC / eval recall@k_list[2] and its test counterpart
CASES = {
    # a stage that only EQUALS the best is a miss: three of them end the loop after stage 3
    "ties": [[(0.60, 0.50), (0.70, 0.61)], [(0.70, 0.90)], [(0.65, 0.1), (0.70, 0.2)], [(0.70, 0.3)], [(0.99, 0.99)]],
    # a late stage beats the best after two misses: the counter starts over and the loop runs all six stages
    "late_winner": [[(0.70, 0.60)], [(0.60, 0.5)], [(0.65, 0.5)], [(0.80, 0.75), (0.79, 0.9)], [(0.70, 0.1)], [(0.80, 0.2)]],
    # scores that never exceed 0: nothing is ever stored, every stage is a miss
    "never_above_zero": [[(0.0, 0.3), (0.0, 0.4)], [(0.0, 0.5)], [(0.0, 0.6)], [(0.5, 0.5)]],
    # always improving: the loop ends with the fifth restart
    "improving": [[(0.50 + 0.05 * s, 0.40 + 0.05 * s), (0.49, 0.99)] for s in range(7)],
    # inside a stage the FIRST epoch that reaches the maximum counts (strict >)
    "epoch_ties": [[(0.55, 0.10), (0.66, 0.20), (0.66, 0.30), (0.60, 0.40)], [(0.66, 0.5), (0.67, 0.6), (0.67, 0.7)],
                   [(0.1, 0.1)], [(0.2, 0.2)], [(0.67, 0.9)]],
    # a first stage at 0 followed by real scores
    "zero_then_scores": [[(0.0, 0.1)], [(0.4, 0.3)], [(0.3, 0.9)], [(0.4, 0.8)], [(0.39, 0.7)]],
}


def lists7(v):
    """A 7-entry metric list whose entry 2 is ``v`` (the only one the book-keeping compares)."""
    return [round(v * f, 6) for f in (0.25, 0.5)] + [v] + [round(min(1.0, v * f), 6) for f in (1.1, 1.2, 1.3, 1.4)]


def run_case(tu, form, stages, out_dir):
    args = SimpleNamespace(path=SimpleNamespace(output=out_dir + os.sep), log_name=f"fixture_{form}", h_hop=H_HOP,
                           load_pretrain_emb=False)
    info = tu.Train_info_record_sw_emb(args) if form == "ctr" else tu.Train_info_record_emb_sw_ndcg(args)
    records, fed = [], []

    def one_stage(epochs):
        info.update_cur_train_info(args, False)
        fed_epochs = []
        for step, (ev, te) in enumerate(epochs):
            esi = tu.Eval_score_info()
            if form == "ctr":
                esi.eval_auc_acc_f1 = [ev, round(ev * 0.9, 6), round(ev * 0.8, 6)]
                esi.test_auc_acc_f1 = [te, round(te * 0.9, 6), round(te * 0.8, 6)]
                fed_epochs.append({"eval": esi.eval_auc_acc_f1, "test": esi.test_auc_acc_f1})
            else:   # [ndcg, recall, precision]
                esi.eval_ndcg_recall_pecision = [lists7(ev * 0.5), lists7(ev), lists7(ev * 0.1)]
                esi.test_ndcg_recall_pecision = [lists7(te * 0.5), lists7(te), lists7(te * 0.1)]
                fed_epochs.append({"eval": {"ndcg": lists7(ev * 0.5), "recall": lists7(ev), "precision": lists7(ev * 0.1)},
                                   "test": {"ndcg": lists7(te * 0.5), "recall": lists7(te), "precision": lists7(te * 0.1)}})
            info.update_score(step, esi)
        info.train_over(0)
        if form == "ctr":
            rec = {"max_eval": info.max_eval_auc, "max_test": info.max_test_auc, "best_pair": list(info.emb_score_auc_tmp[0][H_HOP])}
        else:
            rec = {"max_eval": info.max_eval_recall[2], "max_test": info.max_test_recall[2],
                   "best_pair": list(info.emb_score_recall_tmp[0][2])}
        rec["sw_early_stop"] = info.sw_early_stop
        records.append(rec)
        fed.append(fed_epochs)

    it = iter(stages)
    one_stage(next(it))                       # main.py:35
    for _ in range(5):                        # main.py:39-42
        epochs = next(it, None)
        if epochs is None:
            raise ValueError("case too short for the loop")
        one_stage(epochs)
        if info.sw_early_stop >= 3:
            break
    for lg in (info.logger, info.logger_best):
        for h in list(lg.handlers):
            h.close()
            lg.removeHandler(h)
    return {"form": form, "epochs": fed, "stages": records, "stages_run": len(records)}


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MVIN_REFERENCE", "/root/reference")
    sys.path.insert(0, os.path.join(ref_root, "src", "model", "MVIN"))
    with redirect_stdout(io.StringIO()):
        tu = importlib.import_module("train_util")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for form in ("ctr", "topk"):
            for name, stages in CASES.items():
                padded = list(stages) + [[(0.0, 0.0)]] * 6            # the loop never runs out of made-up stages
                with redirect_stdout(io.StringIO()):
                    case = run_case(tu, form, padded, tmp)
                case["name"] = name
                cases.append(case)
    logging.shutdown()
    with open(OUT, "w") as f:
        json.dump({"max_stages": 5, "patience": 3, "cases": cases}, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
