"""scamd -- Python (ctypes) host side of libsc_engine.so, the MI355X-native engine for the
MCTS + NN self-play hot path of pierric/smart-chess-rust.

The classes mirror the reference's own interfaces for this path so that tests read like the
reference's usage:

  ChessHip.predict / reverse_q   <->  trait Game<S> (src/game.rs:3-15) as implemented by
                                       ChessTS / ChessOnnx (src/backends/torch.rs:89-146)
  SelfPlay                       <->  bin `selfplay` (src/main.rs:155-238): same flag names
  encode_positions               <->  BoardState + _encode (src/chess.rs:665-877)
  encode_steps                   <->  libsmartchess.chess_encode_steps (src/lib.rs:46-128), the trace -> training-tensor step
  encode_steps_torch,            <->  the same, plus ChessDataset's _prepare (py/dataset.py:31-87), as torch tensors on the GPU
  SelfPlay.training_tensors           (from recorded games, or from the self-play trace ring in place)
  score_torch, compare_torch,    <->  scripts/train.py validation_step (loss1, loss2, pi_entropy) and scripts/validate_model.py
  Engine.forward_torch                (total variation, |value1 - value2|) on those tensors, without leaving the GPU
  gather_batch_torch,            <->  DataLoader(ConcatDataset([ChessDataset ...]), shuffle=True, drop_last=True) + _prepare
  ReplayBuffer                        (scripts/train.py:331-353): shuffled trainer-layout minibatches from the compact tensors

  scamd.san (not re-exported)    <->  ValidationDataset (py/dataset.py:90-128): games as SAN movetext (sample.csv, PGN) -> moves and
                                      training tensors, resolved against the legal moves on the GPU

There is NO CPU fallback: importing works anywhere (so the C ABI can be checked), but every
compute entry point raises EngineError when the HIP library or a GPU is missing.
"""
from .binding import EngineError, TERMINATION, encode_move, hip_runtime, hip_runtime_files, lib, lib_path, move_uci, runtime_flags, uci_move  # noqa: F401
from .net import ChessHip, Engine, encode_positions  # noqa: F401
from .training import compare_torch, encode_steps, encode_steps_batch, encode_steps_torch, pack_steps, score_torch  # noqa: F401
from .replay import ReplayBuffer, ReplayIndex, gather_batch_torch  # noqa: F401
from .selfplay import Play, SelfPlay, choose_child, elo, enqueue_interleaved, find_max, play_match, search, write_trace_json  # noqa: F401
from . import binding  # noqa: F401
