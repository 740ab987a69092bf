"""Two networks on the positions of recorded games: how far apart are their policies and values?  The command line of the
reference's scripts/validate_model.py, on the GPU engine (sc_compare_engines): decides whether an exported or re-quantised
network may replace the one it came from.

    python tools/validate_model.py -t TRACE.json [TRACE.json ...] --model1 [N_RES_BLOCKS:]A.scw --model2 [N_RES_BLOCKS:]B.scw
                                   [--games-csv GAMES.csv [--limit N]] [--pgn GAMES.pgn]
                                   [--precision1 {bf16,fp8}] [--precision2 {bf16,fp8}] [--losses] [--device N]

TRACE.json: the trace files this library writes (SelfPlay.write_trace / lib/sc-selfplay; the reference's format).  --games-csv: a
game table with `moves` (SAN movetext) and `winner` columns, as the reference's py/validation/sample.csv (its ValidationDataset
reads the first 10 rows: --limit 10); --pgn: a PGN file of games, from the start position or from a [FEN] header.  Those games are read on the GPU
(scamd.san.encode_san_torch): every ply a position, the visit shares one-hot on the move played.  The sources add up.  Models are
.scw blobs (tools/scw.py, tools/ckpt_to_scw.py); an SCW2 blob carries its own precision.  Prints the policy difference (total
variation per position) and the value difference as mean / std / max / min, and with --losses the validation losses of each
model on the traces' visit shares and outcomes (train.py's val_*_loss1 / val_*_loss2).  torch must be importable: the
positions are encoded into, and scored from, GPU memory."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-t", "--trace", type=str, nargs="+", action="extend")
    ap.add_argument("--games-csv", type=str, help="game table with `moves` (SAN) and `winner` columns")
    ap.add_argument("--limit", type=int, default=None, help="read only the first N rows of --games-csv")
    ap.add_argument("--pgn", type=str, help="PGN file (games from the start position or from a [FEN] header)")
    ap.add_argument("--model1", required=True, type=str, help="[n_res_blocks:]path of an .scw blob")
    ap.add_argument("--model2", required=True, type=str)
    prec_help = "precision an SCW1 (fp32) blob is run in; ignored for an SCW2 blob, which is the fp8 export and says so itself"
    ap.add_argument("--precision1", choices=("bf16", "fp8"), default="bf16", help=prec_help)
    ap.add_argument("--precision2", choices=("bf16", "fp8"), default="bf16", help=prec_help)
    ap.add_argument("--losses", action="store_true", help="also print val_loss1 / val_loss2 of each model on the traces")
    ap.add_argument("--device", type=int, default=0)
    return ap


def model_spec(spec):
    """'[n_res_blocks:]path' -> (n_res_blocks or None, path)"""
    head, sep, tail = spec.partition(":")
    if sep and head.isdigit():
        return int(head), tail
    return None, spec


def load_trace(path):
    """a trace file -> (steps in encode_steps_batch's form, White's result)"""
    with open(path) as f:
        tr = json.load(f)
    steps = [(s[0], [(c[0], int(c[1])) for c in s[2]]) for s in tr["steps"]]
    oc = tr.get("outcome")
    win = 0.0 if not oc or oc.get("winner") is None else 1.0 if oc["winner"] == "White" else -1.0
    return steps, win


def main(argv=None):
    args = parser().parse_args(argv)
    if not args.trace and not args.games_csv and not args.pgn:
        print("No trace file specified.")
        return 0
    import torch  # (first: libsc_engine.so then binds to the HIP runtime torch loaded)
    sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))
    import scamd

    specs = [model_spec(args.model1), model_spec(args.model2)]
    for nb, path in specs:   # before any engine exists
        if nb is not None and nb != eng_blocks(path):
            raise SystemExit(f"{path}: the blob holds {eng_blocks(path)} residual blocks, the model spec says {nb}")
    import scamd.san
    san_games, san_winners, san_fens = [], [], []
    if args.games_csv:
        san_games, san_winners = scamd.san.read_games_csv(args.games_csv, args.limit)
        san_fens = [None] * len(san_games)
    if args.pgn:
        g, w, fens = scamd.san.read_pgn(args.pgn, setup=True)   # games from a [FEN] position are read too
        san_games, san_winners, san_fens = san_games + g, san_winners + w, san_fens + fens
    engines = []
    try:
        for (nb, path), prec in zip(specs, (args.precision1, args.precision2)):
            engines.append(scamd.Engine(weights=path, device=args.device, precision=prec))
        parts = []
        if args.trace:
            games, wins = zip(*(load_trace(p) for p in args.trace))
            t = scamd.encode_steps_torch(list(games), layout="reference", dist="legal", engine=engines[0], outcomes=list(wins))
            if (t["status"] != 0).any():
                bad = [(args.trace[g], int(s)) for g, s in enumerate(t["status"]) if s]
                raise SystemExit(f"traces that do not replay (sc_encode_steps status codes): {bad}")
            parts.append(t)
        if san_games:
            t = scamd.san.encode_san_torch(san_games, san_winners, device=args.device, engine=engines[0], fens=san_fens)
            if (t["status"] != 0).any():
                bad = [(g + 1, int(s)) for g, s in enumerate(t["status"]) if s]
                raise SystemExit(f"games that do not parse (game number, sc_encode_san_device status code): {bad}")
            parts.append(t)
        t = parts[0] if len(parts) == 1 else {k: torch.cat([q[k] for q in parts]) for k in ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")}
        print("Running inference...")
        r = scamd.compare_torch(engines[0], engines[1], t)
        print("policy difference:", {k: r["tv_" + k] for k in ("mean", "std", "max", "min")})
        print("value difference:", {k: r["dv_" + k] for k in ("mean", "std", "max", "min")})
        if args.losses:
            for name, eng in zip(("model1", "model2"), engines):
                s = scamd.score_torch(eng, t)
                print(f"{name}:", {"val_loss1": s["loss1"], "val_loss2": s["loss2"], "pi_entropy": s["pi_entropy"], "non_finite": s["n_nonfinite"]})
    finally:
        for eng in engines:
            eng.close()
    return 0


def eng_blocks(path):
    """residual blocks of an .scw blob (tools/scw.py write_scw: magic, then n_blocks as a little-endian uint32)"""
    with open(path, "rb") as f:
        head = f.read(8)
    if head[:4] not in (b"SCW1", b"SCW2"):
        raise SystemExit(f"{path}: not an .scw blob")
    return int.from_bytes(head[4:8], "little")


if __name__ == "__main__":
    sys.exit(main())
