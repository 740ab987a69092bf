"""Match play against an outside opponent, what its tests share: the colour rule of sc_selfplay_set_external, the trace such a handle
must give for a reference game, and the script that makes a ScriptedOpponent replay one side of reference games."""


def engine_white(colours, k):
    """is the engine White in handle-local game k?  colours 0: always, 1: in the even games, 2: never"""
    return colours == 0 or (colours == 1 and k % 2 == 0)


def engine_moves_ply(colours, k, i):
    """does the engine move at ply i (from the start position) of game k?"""
    return (i % 2 == 0) == engine_white(colours, k)


def pushed_step(step):
    """a reference step as the device records it when the move was pushed: one visit on the move, every value 0"""
    move, _q, kids = step
    return (move, 0.0, [(m, 1 if m == move else 0, 0.0, 0.0) for m, *_ in kids])


def expected_steps(ref_steps, colours, k):
    """the steps of game k on an external handle whose opponent replays the reference game's other side"""
    return [s if engine_moves_ply(colours, k, i) else pushed_step(s) for i, s in enumerate(ref_steps)]


def script_table(orc, games, colours, form="fen"):
    """{(k, position line): uci} for the opponent's plies of the reference games {k: steps} -- keyed by game: two games can pass
    through one position (the start position) and go on differently"""
    table = {}
    for k, steps in games.items():
        st = orc.State()
        played = []
        for i, (move, _q, _kids) in enumerate(steps):
            if not engine_moves_ply(colours, k, i):
                line = "position fen " + st.fen() if form == "fen" else "position startpos" + (" moves " + " ".join(played) if played else "")
                table[k, line] = move
            st.push(move)
            played.append(move)
    return table


def legal_replay(orc, steps):
    """every step's move is legal and its children are the legal moves in the generator's order -> the final State"""
    st = orc.State()
    for i, (move, _q, kids) in enumerate(steps):
        legal = st.legal_uci()
        assert move in legal, (i, move)
        assert [c[0] for c in kids] == legal, (i, move)
        st.push(move)
    return st
