"""Host-side token <-> chemistry glue for the 'chartok_coords' output format.

Mirrors the interface of the reference's CharTokenizer (reference MolNexTR/tokenization.py:330-515,
NodeTokenizer :112-199) for the inference direction only: ids -> raw SMILES, atom symbols, coordinates and
the decoder positions whose hidden states feed the bond head. Stays on the host by design (BASELINE
north_star); the grammar rule it defines (`get_output_mask`) is ALSO compiled into the HIP decode step
(csrc/decoder.hip) — `tests/test_tokenizer.py` checks both against the golden truth table.

Token id map (vocab/vocab_chars.json, 101 symbols): 0 <pad>, 1 <sos>, 2 <eos>, 3 <unk>, 4 <mask>,
5..100 characters, x-bins [101,165), y-bins [165,229); coordinate = (id - base) / 63.
"""
import json
import os
import re

PAD_ID, SOS_ID, EOS_ID, UNK_ID, MASK_ID = 0, 1, 2, 3, 4
PAD, SOS, EOS, UNK, MASK = "<pad>", "<sos>", "<eos>", "<unk>", "<mask>"

_VOCAB_DEFAULT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vocab", "vocab_chars.json")


# The atom-wise SMILES pattern published with SmilesPE / the Molecular Transformer (Schwaller et al.): a bracket atom, a
# two-letter halogen, an organic-subset atom (aromatic ones included), a bond / branch / charge / dot symbol, a two-digit
# ring closure "%nn", or one digit. Restated from the publication; tests pin it on fixtures made by the reference.
_ATOMWISE = re.compile(r"(\[[^\]]+]|Br?|Cl?|N|O|S|P|F|I|b|c|n|o|s|p|\(|\)|\.|=|#|-|\+|\\|\/|:|~|@|\?|>|\*|\$|\%[0-9]{2}|[0-9])")


def atomwise_tokenizer(smi):
    """SMILES -> list of atom-wise tokens (characters the pattern does not know are dropped, as re.findall does)."""
    return _ATOMWISE.findall(smi)


class CharTokenizer:
    """Character-level tokenizer with separate x / y coordinate bins (sep_xy=True)."""

    def __init__(self, input_size=64, path=None, sep_xy=True, continuous_coords=False, debug=False):
        with open(path or _VOCAB_DEFAULT) as f:
            self.stoi = json.load(f)
        self.itos = {i: s for s, i in self.stoi.items()}
        self.maxx = self.maxy = int(input_size)
        self.sep_xy = sep_xy
        self.continuous_coords = continuous_coords
        self.special_tokens = [PAD, SOS, EOS, UNK, MASK]
        self.debug = debug
        if not sep_xy or continuous_coords:
            raise NotImplementedError("the MolNexTR inference config uses sep_xy=True, discrete coordinates")

    # -- sizes / id classes (reference tokenization.py:125-170) --------------------------------
    def __len__(self):
        return self.offset + self.maxx + self.maxy

    @property
    def offset(self):
        return len(self.stoi)

    @property
    def output_constraint(self):
        return True

    def is_x(self, i):
        return self.offset <= i < self.offset + self.maxx

    def is_y(self, i):
        return self.offset + self.maxx <= i

    def is_symbol(self, i):
        return len(self.special_tokens) <= i < self.offset or i == UNK_ID

    @staticmethod
    def is_atom_token(token):
        return token.isalpha() or token.startswith("[") or token == "*" or token == UNK

    def is_atom(self, i):
        return self.is_symbol(i) and self.is_atom_token(self.itos[i])

    def id_to_x(self, i):
        return (i - self.offset) / (self.maxx - 1)

    def id_to_y(self, i):
        return (i - self.offset - self.maxx) / (self.maxy - 1)

    def x_to_id(self, x):
        return self.offset + round(x * (self.maxx - 1))

    def y_to_id(self, y):
        return self.offset + self.maxx + round(y * (self.maxy - 1))

    # -- decode-time grammar (reference tokenization.py:383-392) --------------------------------
    def get_output_mask(self, prev_id):
        """True = forbidden as the next token. After an x-bin only y-bins; after a y-bin no coordinate bins."""
        V, x0, y0 = len(self), self.offset, self.offset + self.maxx
        if self.is_x(prev_id):
            return [t < y0 for t in range(V)]
        if self.is_y(prev_id):
            return [t >= x0 for t in range(V)]
        return [False] * V

    # -- SMILES -> label ids (reference tokenization.py:429-462) ---------------------------------
    def smiles_to_sequence(self, smiles, coords=None, mask_ratio=0, atom_only=False):
        """(labels, indices): '<sos>', every character of every atom-wise token ('<unk>' outside the vocabulary), after
        each atom token its x and y — '<mask>' twice with mask_ratio=1, the bins of coords[k] when coords is given, nothing
        otherwise — then '<eos>'; indices[k] = position of the last id of atom k's group. mask_ratio is honoured for 0 and 1
        only (anything between draws random numbers in the reference), and so is an atom beyond len(coords)."""
        if mask_ratio not in (0, 1):
            raise ValueError("mask_ratio must be 0 or 1: partial masking is random in the reference and not restated")
        labels, indices, atom_idx = [SOS_ID], [], -1
        for token in atomwise_tokenizer(smiles):
            if atom_only and not self.is_atom_token(token):
                continue
            labels.extend(self.stoi.get(c, UNK_ID) for c in token)
            if self.is_atom_token(token):
                atom_idx += 1
                if mask_ratio == 1:
                    labels += [MASK_ID, MASK_ID]
                elif coords is not None:
                    if atom_idx >= len(coords):
                        raise ValueError("fewer coordinates than atoms (the reference draws random ones)")
                    x, y = coords[atom_idx]
                    assert 0 <= x <= 1 and 0 <= y <= 1
                    labels += [self.x_to_id(x), self.y_to_id(y)]
                indices.append(len(labels) - 1)
        labels.append(EOS_ID)
        return labels, indices

    # -- ids -> {smiles, symbols, coords, indices} (reference tokenization.py:464-515) ----------
    def _atom_span_end(self, seq, i):
        """End (exclusive) of the atom token starting at i: '[...]' up to the closing bracket or the first
        non-symbol id; 'Cl'/'Br' as two characters; otherwise one character."""
        first = self.itos[seq[i]]
        n = len(seq)
        if first == "[":
            j = i + 1
            while j < n and self.is_symbol(seq[j]):
                j += 1
                if self.itos[seq[j - 1]] == "]":
                    break
            return j
        if i + 1 < n and self.is_symbol(seq[i + 1]) and (first, self.itos[seq[i + 1]]) in (("C", "l"), ("B", "r")):
            return i + 2
        return i + 1

    def sequence_to_smiles(self, sequence):
        seq = list(sequence)
        n = len(seq)
        pieces, coords, symbols, indices = [], [], [], []
        i = 0
        while i < n:
            t = seq[i]
            if t == EOS_ID or t == PAD_ID:
                break
            if self.is_x(t) or self.is_y(t):
                i += 1
            elif not self.is_atom(t):
                pieces.append(self.itos[t])
                i += 1
            else:
                j = self._atom_span_end(seq, i)
                token = "".join(self.itos[seq[k]] for k in range(i, j))
                pieces.append(token)
                # an atom is kept only if "x y <next token>" all exist after it (the hidden state at the
                # position after y feeds the bond head)
                if j + 2 < n and self.is_x(seq[j]) and self.is_y(seq[j + 1]):
                    coords.append([self.id_to_x(seq[j]), self.id_to_y(seq[j + 1])])
                    symbols.append(token)
                    indices.append(j + 2)
                    i = j + 2
                else:
                    i = j
        return {"smiles": "".join(pieces), "symbols": symbols, "indices": indices, "coords": coords}


def coords_labels(tok, smiles_list, max_len: int):
    """Labels of coordinate prediction for known structures: smiles_to_sequence(s, mask_ratio=1) of every SMILES (reference
    dataset.py:459-464) cut to max_len ids (dataset.py:473) and padded with '<pad>' to a common L >= 2. Returns
    (labels int32 [n, L], cut bool [n]): cut marks the rows the cut shortened, which have lost their '<eos>'."""
    import numpy as np
    seqs = [tok.smiles_to_sequence(s, mask_ratio=1)[0] for s in smiles_list]
    cut = np.array([len(q) > max_len for q in seqs], dtype=bool)
    labels = np.zeros((len(seqs), max(2, min(max_len, max((len(q) for q in seqs), default=2)))), dtype=np.int32)     # '<pad>' = 0
    for i, q in enumerate(seqs):
        q = q[:max_len]
        labels[i, :len(q)] = q
    return labels, cut


def get_tokenizer(args=None):
    """{'chartok_coords': CharTokenizer}; mirrors reference tokenization.py:518-543 for the inference formats."""
    bins = getattr(args, "coord_bins", 64) if args is not None else 64
    path = getattr(args, "vocab_file", None) if args is not None else None
    return {"chartok_coords": CharTokenizer(bins, path, sep_xy=True)}
