"""Records tests/golden/textpath_bert.npz: tests/bert_textpath_case.run() on an MI355X with the engine as it was before
the text calls took the Unigram tokenizer (the commit "Add cross-encoder reranking of search results on the GPU").
Run on the GPU with that commit's package first on the path, its library built:
    PYTHONPATH=<checkout of that commit> python tests/golden/make_bert_textpath_golden.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(HERE))  # tests/, after the checkout named by PYTHONPATH
sys.path.append(os.path.dirname(os.path.dirname(HERE)))  # oracle/ (and this tree's package, which must NOT win)

import bert_textpath_case  # noqa: E402
import voitta_rag_amd  # noqa: E402


def main():
    where = os.path.dirname(os.path.abspath(voitta_rag_amd.__file__))
    print("package:", where)
    assert os.path.dirname(where) != os.path.dirname(os.path.dirname(HERE)), "this tree's package, not the earlier one"
    out = bert_textpath_case.run()
    np.savez_compressed(sys.argv[1], **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
