/* Nothing: the reference's simulator includes this header and uses nothing from it. */
